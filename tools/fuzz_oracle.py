#!/usr/bin/env python3
"""tools/fuzz_oracle.py [cases] [seed] [kinds] [--subject gpu] -- randomized differential run of a SUBJECT against the LIVE REFERENCE
builds under oracle/_ref (oracle/ref/build_ref.sh): one function per family draws a case, runs the reference's own code (po.RefHost(),
po.csref(), libcompref.so, libresizableref.so) and the subject on the same inputs with identically pre-filled destinations, and compares the
whole destination arrays, row padding included.  The subject is the CPU oracle (oracle/lives_oracle.c, default) or the GPU library
(lives_amd.ops, --subject gpu).  TEST / DEBUG TOOL.  It reads oracle/_ref/*.so only, nothing from the reference's source tree.

`cases` is the number of cases PER FAMILY (stateful families: a tenth of it, at least 1, sequences of 5-12 frames).  One line per family
(compared / skipped / mismatching / masked bytes), then a summary line `fuzz_oracle: ...` a test can parse; run() returns the same numbers.

Sizes and parameters follow tools/fuzz_ops.py for the matching kind (FUZZ_OPS_RANGES: the line of fuzz_ops.py a range was copied from is
kept beside it, tests/test_oracle_live.py checks that it still stands there); families without a fuzz_ops kind use the largest sizes of
tests/test_gpu_parity.py, capped at 300x120.  Odd sizes and 1-pixel sides are drawn wherever the entry point takes them."""
import ctypes
import os
import re
import shutil
import sys
import tempfile
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import pyoracle as po  # noqa: E402

P = po.P
vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double

# ---- ranges shared with tools/fuzz_ops.py: kind -> (the line as it stands in fuzz_ops.py, the numbers of that line) ----------------------
FUZZ_OPS_RANGES = {
    "swizzle": ("w, h = int(rng.integers(1, 500)), int(rng.integers(1, 60))", (1, 500, 1, 60)),
    "k2": ("w, h = 2 * int(rng.integers(1, 200)), int(rng.integers(1, 100))", (1, 200, 1, 100)),
    "gamma": ("w, h = int(rng.integers(2, 300)), int(rng.integers(2, 100))", (2, 300, 2, 100)),
    "rgb2yuv": ("w, h = int(rng.integers(1, 200)), int(rng.integers(1, 80))", (1, 200, 1, 80)),
    "yuv2rgb": ("w, h = int(rng.integers(1, 200)), int(rng.integers(1, 80))", (1, 200, 1, 80)),
    "repack": ("w, h = 2 * int(rng.integers(1, 150)), 2 * int(rng.integers(1, 60))", (1, 150, 1, 60)),
    "repack411": ("w, h = 4 * int(rng.integers(1, 120)), int(rng.integers(1, 80))", (1, 120, 1, 80)),
    "yuv411": ("wm, h = int(rng.integers(1, 200)), int(rng.integers(1, 60))", (1, 200, 1, 60)),
    "rgb411": ("w, h = int(rng.integers(4, 700)), int(rng.integers(1, 60))", (4, 700, 1, 60)),
    "blend": ("w, h = int(rng.integers(1, 300)), int(rng.integers(1, 100))", (1, 300, 1, 100)),
    "luma": ("w, h = int(rng.integers(1, 300)), int(rng.integers(1, 100))", (1, 300, 1, 100)),
    "multi": ("w, h = int(rng.integers(1, 300)), int(rng.integers(1, 100))", (1, 300, 1, 100)),
    "colorkey": ("w, h = int(rng.integers(1, 300)), int(rng.integers(1, 100))", (1, 300, 1, 100)),
    "mirror": ("w, h = int(rng.integers(1, 300)), int(rng.integers(1, 120))", (1, 300, 1, 120)),
    "softlight": ("w, h = 2 * int(rng.integers(2, 150)), 2 * int(rng.integers(2, 70))", (2, 150, 2, 70)),
    "edge": ("w, h = int(rng.integers(4, 260)), int(rng.integers(4, 140))", (4, 260, 4, 140)),
    "transition": ("w, h = int(rng.integers(2, 300)), int(rng.integers(2, 120))", (2, 300, 2, 120)),
    "slide": ("w, h = int(rng.integers(1, 300)), int(rng.integers(1, 100))", (1, 300, 1, 100)),
    "deint": ("w, h = int(rng.integers(1, 200)), int(rng.integers(1, 80))", (1, 200, 1, 80)),
    "bytelut": ("w, h = int(rng.integers(1, 400)), int(rng.integers(1, 80))", (1, 400, 1, 80)),
    "tsplit": ("w, h = int(rng.integers(1, 300)), int(rng.integers(1, 100))", (1, 300, 1, 100)),
}
PAD_ALIGNS = [1, 4, 8, 16, 32]           # fuzz_ops.py fr(): rowstride = align(w * ps, one of these) + 0..2 of it
LUMA_FN = {1: "luma overlay", 2: "luma underlay", 3: "negative luma overlay", 4: "averaged luma overlay"}
MULTI_FN = ["blend_multiply", "blend_screen", "blend_darken", "blend_lighten", "blend_overlay", "blend_dodge", "blend_burn"]
GAMMA_IDS = [po.GAMMA_LINEAR, po.GAMMA_SRGB, po.GAMMA_BT709, po.GAMMA_MONITOR]
RS_PALS = [1, 2, 3, 4, 5, 512, 513, 522, 544, 545, 564, 565, 588, 589, 595]
# K1: the call modes in which the reference produces the intended permutation (oracle/ref/gen_golden.py `canon`): (op, in place, nfx_threads)
K1_CANON = [("swap3", 1, 2), ("swap3addpost", 0, 1), ("swap3addpost", 0, 2), ("swap3addpre", 0, 2), ("swap3postalpha", 1, 2),
            ("swap3prealpha", 1, 2), ("addpost", 0, 2), ("addpre", 0, 2), ("swap3delpost", 0, 2), ("delpost", 0, 2), ("swap3delpre", 0, 2),
            ("delpre", 0, 2), ("swap3", 1, 1), ("swap3postalpha", 1, 1), ("swap3prealpha", 1, 1)]


def k1_slice0_swallows(h, nthr):
    """:9271-9283 with nfx_threads = 2: slice 1 starts at row CEIL(h / 2, 4); where that is past row h - 4 slice 0 takes the whole frame and the rows of slice 1
    are converted twice (in place: swapped back)"""
    xd = -(-h // (2 * 4)) * 4 if nthr == 2 else h
    return nthr == 2 and xd < h and xd > h - 4

# ---- exceptions: family -> [(kind, predicate over the drawn case, reason, reference line or docs/QUIRKS.md id)] ---------------------------
# kind "never": a combination the reference is broken on or does not offer (refused by the library / "unpinned" in tests/golden/manifest.json);
#               the driver redraws until no such predicate holds.
# kind "mask":  bytes whose reference value is undefined, named by the manifest; the predicate says whether the case has any, the family's
#               function builds the mask and states the most bytes it may cover (run() counts a case whose mask is larger as a failure).
# A draw outside this table on which the reference returns non-zero, or which the subject refuses, is a mismatch.
EXCEPTIONS = {
    "k1": [("never", lambda c: c["op"] in ("swap4", "swapprepost"), "reference-broken in every mode", "K1-b"),
           ("never", lambda c: c["op"] == "delpre" and not c["lut"], "the no-LUT body copies the same pixel", "K1-b"),
           ("never", lambda c: c["op"] == "swap3" and c["nthr"] == 1, "the one-thread body walks a third of the row and never writes G", "K1-a"),
           ("never", lambda c: c["inplace"] and k1_slice0_swallows(c["h"], c["nthr"]), "in place with two threads: slice 0 swallows the frame at heights 5-7 and 9-11, "
            "the rows of slice 1 are swapped twice", "K1-c, src/colourspace.c:9271-9283")],
    "k2": [("never", lambda c: not c["is422"] and c["h"] < 2, "4:2:0 needs a chroma row", "lgpu_yuv420p_to_rgb refuses"),
           ("mask", lambda c: not c["is422"], "row 0 at odd x (out-of-bounds table index), last row at odd x (never written, even heights)", "K2-a / K2-c"),
           ("mask", lambda c: not c["is422"] and (c["which"] & 1), "unclamped 4:2:0 rows 1..h-2 are written one byte early: rows 0 and h-1, the last "
            "column and pixel (1, 0) overlap their neighbours", "K2-f, src/colourspace.c:3707")],
    "k2_lut16": [("never", lambda c: not c["is422"] and c["h"] < 2, "4:2:0 needs a chroma row", "lgpu_yuv420p_to_rgb refuses"),
                 ("mask", lambda c: not c["is422"], "as k2", "K2-a / K2-c / K2-f")],
    "k4": [("never", lambda c: c["out_fmt"] >= 4 and c["in_order"] == 2, "ARGB -> 4:2:0 / 4:2:2 reads the wrong bytes", "src/colourspace.c:6353"),
           ("never", lambda c: c["out_fmt"] >= 2 and (c["w"] & 1), "subsampled targets take an even width", "lgpu_rgb_to_yuv refuses"),
           ("never", lambda c: c["out_fmt"] == 4 and (c["h"] & 1), "4:2:0 takes an even height", "lgpu_rgb_to_yuv refuses"),
           ("never", lambda c: c["out_fmt"] >= 2 and not c["compact"], "the reference's 4:2:0 / 4:2:2 / UYVY row arithmetic only works on compact rows", "K4-c")],
    "k4_lut16": [("mask", lambda c: True, "rgb2uyvy_with_gamma / rgb2yuyv_with_gamma index the 65536-entry LUT with (table sum) >> 8 unchecked: a chroma sum of "
                  "256.0 or more (or below 0) reads outside the table", "K4-g, src/colourspace.c:2146-2158, :2194-2208")],
    "k3": [("never", lambda c: c["in_fmt"] == 1 and c["out_order"] == 2, "planar -> ARGB32 subtracts the output stride twice", "src/colourspace.c:7475-7476"),
           ("never", lambda c: c["in_fmt"] == 1 and c["out_order"] == 1 and not c["out_alpha"], "planar -> BGR24 steps 4 bytes per pixel", "src/colourspace.c:7313"),
           ("never", lambda c: c["in_fmt"] >= 2 and (c["stride"] & 3), "UYVY / YUYV rows are stepped in whole macropixels (irow / 4)", "K3-c, src/colourspace.c:6677")],
    "blend_luma": [("never", lambda c: c["subject"] == "gpu" and c["ps"] == 4 and ((c["stride1"] | c["stride2"]) & 3), "GPU subject only, a contract of the library and no defect of the "
                    "reference: lgpu_blend_luma takes 4-byte pixels on rows that are multiples of 4 bytes only (tools/fuzz_ops.py counts such draws as declined); the "
                    "oracle is compared at every rowstride", "include/lives_gpu.h, buffer alignment")],
    "repack": [("never", lambda c: c["ip"] == 522 and c["op"] in (564, 565), "the reference's functions overrun; own specification", "docs/SPECS.md evident intent")],
    "chroma_up": [("mask", lambda c: c["pad"] == 0, "compact chroma planes: the last pixel of the rows fed by the last chroma row reads one sample past the plane",
                   "po.chroma_up_mask, src/colourspace.c:10715-10873")],
    "mirror": [("never", lambda c: not c["inplace"], "out of place the reference leaves rows / pixels unwritten; the fixtures are in place", "mirrors.c:26-122"),
               ("mask", lambda c: True, "stray writes: pixel `width` of each row for even widths, row `height`", "mirrors.c:26-122")],
    "deinterlace": [("never", lambda c: c["stride"] < (c["w"] + 2) // 3 * 3 * c["ps"], "rows too short for (w + 2) / 3 * 3 pixels", "deinterlace.c:45-308"),
              ("never", lambda c: c["pal"] == 5 and not c["inplace"], "ARGB32 is pinned in place only", "tests/golden/manifest.json deinterlace.npz")],
}


def excluded(family, case):
    return any(kind == "never" and pred(case) for (kind, pred, _r, _w) in EXCEPTIONS.get(family, ()))


def masked(family, case):
    return any(kind == "mask" and pred(case) for (kind, pred, _r, _w) in EXCEPTIONS.get(family, ()))


class quiet_stderr:
    """the reference announces some initialisations on stderr (init_gamma_tx, the dissolve mask): keep them out of the report"""

    def __enter__(self):
        sys.stderr.flush()
        self.keep, self.null = os.dup(2), os.open(os.devnull, os.O_WRONLY)
        os.dup2(self.null, 2)

    def __exit__(self, *a):
        os.dup2(self.keep, 2)
        os.close(self.keep)
        os.close(self.null)


# ---- buffers ------------------------------------------------------------------------------------------------------------------------------
def guarded(shape, fill=None, rng=None, dtype=np.uint8):
    """a C-contiguous 2-D array inside a larger backing buffer: the reference's reads past a plane stay inside memory this process owns"""
    rows, cols = shape
    back = np.zeros((rows + 8) * max(cols, 1) + 256, dtype)
    back[:] = 0x3C
    a = back[4 * max(cols, 1) + 128:4 * max(cols, 1) + 128 + rows * cols].reshape(rows, cols)
    if rng is not None:
        a[:] = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    elif fill is not None:
        a[:] = fill
    return a


def gcopy(a):
    b = guarded(a.shape)
    b[:] = a
    return b


# what one drawn unit of FUZZ_OPS_RANGES is in pixels and rows, where it is not a pixel and a row: "w, h = 2 * int(..), .." draws pixel pairs
GEOMETRY_UNITS = {"k2": (2, 1), "repack": (2, 2), "repack411": (4, 1), "yuv411": (4, 1), "softlight": (2, 2)}


class Draw:
    """fixed: an optional (width, height) in pixels and rows that every geometry draw of a case returns in place of a random one (everything else is still drawn):
    the comparison at one given size, e.g. the widths beyond the ranges above that tests/test_wide_frames.py runs"""

    def __init__(self, rng, fixed=None):
        self.rng, self.fixed = rng, fixed

    def i(self, lo, hi):
        return int(self.rng.integers(lo, hi))

    def wh(self, kind):
        a, b, c, d = FUZZ_OPS_RANGES[kind][1]
        if self.fixed is not None:
            ux, uy = GEOMETRY_UNITS.get(kind, (1, 1))
            assert self.fixed[0] % ux == 0 and self.fixed[1] % uy == 0 and self.fixed[0] >= a * ux and self.fixed[1] >= c * uy, "%s draws no %dx%d" % (kind, self.fixed[0], self.fixed[1])
            return self.fixed[0] // ux, self.fixed[1] // uy
        return self.i(a, b), self.i(c, d)

    def geometry(self, a, b, c, d):
        """the families that draw their own ranges: width in [a, b), height in [c, d)"""
        if self.fixed is not None:
            assert self.fixed[0] >= a and self.fixed[1] >= c, "no %dx%d below %dx%d" % (self.fixed[0], self.fixed[1], a, c)
            return self.fixed
        return self.i(a, b), self.i(c, d)

    def stride(self, w, ps, extra=None):
        al = int(self.rng.choice(PAD_ALIGNS))
        return (w * ps + al - 1) // al * al + (self.i(0, 3) * al if extra is None else extra)

    def fr(self, w, h, ps, extra=None, stride=None, rows=None):
        a = guarded((h if rows is None else rows, self.stride(w, ps, extra) if stride is None else stride), rng=self.rng)
        if ps == 4 and self.rng.random() < 0.5:
            al = a[:, 3::4]
            al[self.rng.random(al.shape) < 0.6] = 255
        return a


# ---- subjects -----------------------------------------------------------------------------------------------------------------------------
class Refused(Exception):
    pass


def _rc(r, what):
    if r != 0:
        raise Refused("%s returned %d" % (what, r))


class OracleSubject:
    name = "oracle"

    def __init__(self):
        self.o = po.oracle()
        self.o.orc_get_resizable.argtypes = [ctypes.POINTER(ci)]

    def swizzle(self, op, src, dst, w, h, lut):
        _rc(self.o.orc_swizzle(op, 0, P(src), src.strides[0], P(dst), dst.strides[0], w, h, P(lut)), "orc_swizzle")

    def k2(self, Y, U, V, dst, w, h, opsz, is422, which, q, lut16=None):
        st = (ci * 3)(Y.strides[0], U.strides[0], V.strides[0])
        fn = self.o.orc_yuv420p_to_rgb_lut16 if lut16 is not None else self.o.orc_yuv420p_to_rgb
        _rc(fn(P(Y), P(U), P(V), st, U.size, V.size, P(dst), dst.strides[0], w, h, opsz, 0, is422, which, q, P(lut16), 0), "orc_yuv420p_to_rgb")

    def gamma_apply(self, pix, x, y, rw, rh, ps, af, lut):
        self.o.orc_gamma_apply(vp(pix.ctypes.data + y * pix.strides[0] + x * ps), pix.strides[0], rw, rh, ps, af, P(lut))

    def gamma_lut8(self, fileg, f, t, sg):
        lut = np.zeros(256, np.uint8)
        return self.o.orc_gamma_lut8(fileg, f, t, sg, P(lut)), lut

    def gamma_lut16(self, fileg, f, t, sg):
        lut = np.zeros(65536, np.uint16)
        return self.o.orc_gamma_lut16(fileg, f, t, sg, P(lut)), lut

    def rgb_to_yuv(self, src, planes, w, h, in_order, in_alpha, out_fmt, out_alpha, which):
        pp, ss = po.planes_args(planes)
        _rc(self.o.orc_rgb_to_yuv(P(src), src.strides[0], w, h, in_order, in_alpha, ctypes.addressof(pp), ctypes.addressof(ss), out_fmt, out_alpha, which), "orc_rgb_to_yuv")

    def rgb_to_yuv_lut16(self, src, dst, w, h, order, alpha, fmt, unc, lut):
        _rc(self.o.orc_rgb_to_yuv_lut16(P(src), src.strides[0], w, h, order, alpha, P(dst), dst.strides[0], fmt, unc, P(lut)), "orc_rgb_to_yuv_lut16")

    def yuv_to_rgb(self, planes, dst, w, h, in_fmt, in_alpha, out_order, out_alpha, which):
        pp, ss = po.planes_args(planes)
        _rc(self.o.orc_yuv_to_rgb(ctypes.addressof(pp), ctypes.addressof(ss), w, h, in_fmt, in_alpha, P(dst), dst.strides[0], out_order, out_alpha, which), "orc_yuv_to_rgb")

    def yuv_repack(self, ip, op, src, dst, w, h, unc, sampling):
        sp, ss = po.planes_args(src)
        dp, ds = po.planes_args(dst)
        _rc(self.o.orc_yuv_repack(ip, op, ctypes.addressof(sp), ctypes.addressof(ss), ctypes.addressof(dp), ctypes.addressof(ds), w, h, unc, sampling), "orc_yuv_repack")

    def yuv411_to_rgb(self, src, wm, h, dst, order, oa, uncl):
        _rc(self.o.orc_yuv411_to_rgb(P(src), wm, h, P(dst), dst.strides[0], order, oa, uncl), "orc_yuv411_to_rgb")

    def rgb_to_yuv411(self, src, w, h, order, ia, dst, uncl):
        _rc(self.o.orc_rgb_to_yuv411(P(src), src.strides[0], w, h, order, ia, P(dst), uncl), "orc_rgb_to_yuv411")

    def yuv_yuv_tables(self):
        t = [np.zeros(256, np.uint8) for _ in range(4)]
        self.o.orc_yuv_yuv_tables(*[P(x) for x in t])
        return t

    def premult_yuv_tables(self):
        t = [np.zeros((256, 256), np.uint8) for _ in range(4)]
        self.o.orc_premult_yuv_tables(*[P(x) for x in t])
        return t

    def blend_chroma(self, s1, s2, dst, w, h, ps, af, bf):
        self.o.orc_blend_chroma(P(s1), s1.strides[0], P(s2), s2.strides[0], P(dst), dst.strides[0], w, h, ps, af, bf)

    def blend_luma(self, kind, s1, s2, dst, w, h, ps, order, thr):
        self.o.orc_blend_luma(kind, P(s1), s1.strides[0], P(s2), s2.strides[0], P(dst), dst.strides[0], w, h, ps, order, thr, int(s1 is dst))

    def blend_multi(self, kind, s1, s2, dst, w, h, is_bgr, bf):
        self.o.orc_blend_multi(kind, P(s1), s1.strides[0], P(s2), s2.strides[0], P(dst), dst.strides[0], w, h, is_bgr, bf)

    def colorkey(self, s0, s1, dst, w, h, is_bgr, delta, opac, col):
        self.o.orc_colorkey(P(s0), s0.strides[0], P(s1), s1.strides[0], P(dst), dst.strides[0], w, h, is_bgr, delta, opac, col[0], col[1], col[2], 0)

    def mirror(self, mode, src, dst, w, h, ps):
        self.o.orc_mirror(mode, P(src), src.strides[0], P(dst), dst.strides[0], w, h, ps)

    def softlight(self, src, dst, w, h, pal, unc):
        self.o.orc_softlight_y(P(src[0]), src[0].strides[0], P(dst[0]), dst[0].strides[0], w, h, unc)
        dims = [(w, h)] + [(w >> 1 if pal in (512, 513, 522) else w, h >> 1 if pal in (512, 513) else h)] * 2 + ([(w, h)] if pal == 545 else [])
        # the oracle has the Y entry only (orc_softlight_y); the other planes are copied through HERE, as softlight.c does, so that the whole-plane comparison has
        # something to hold against the reference: for this subject planes 1.. check this tool, not lives_oracle.c (for the GPU subject they check lgpu_softlight)
        for i in range(1, len(src)):
            dst[i][:dims[i][1], :dims[i][0]] = src[i][:dims[i][1], :dims[i][0]]

    def edge(self, src, dst, w, h, pal, mode):
        m16 = np.zeros(w * h, np.int16)
        self.o.orc_edge(P(src), src.strides[0], P(dst), dst.strides[0], w, h, pal, mode, P(m16), int(src is dst))

    def transition(self, t, s1, s2, dst, w, h, ps, amt):
        self.o.orc_transition(t, P(s1), s1.strides[0], P(s2), s2.strides[0], P(dst), dst.strides[0], w, h, ps, amt)

    def dissolve(self, s1, s2, dst, w, h, ps, seed, amt):
        mask = np.zeros(w * h, np.float32)
        self.o.orc_dissolve_mask(seed, w, h, mask.ctypes.data)
        self.o.orc_dissolve(P(s1), s1.strides[0], P(s2), s2.strides[0], P(dst), dst.strides[0], w, h, ps, mask.ctypes.data, amt)

    def slide_over(self, s1, s2, dst, w, h, ps, tv, dirn, mvl, mvu):
        self.o.orc_slide_over(P(s1), s1.strides[0], P(s2), s2.strides[0], P(dst), dst.strides[0], w, h, ps, tv, dirn, mvl, mvu)

    def deinterlace(self, src, dst, w, h, pal):
        _rc(self.o.orc_deinterlace(P(src), src.strides[0], P(dst), dst.strides[0], w, h, pal), "orc_deinterlace")

    def script_fx(self, kind, pal, prm, src, dst, w, h, ps):
        luts = np.zeros((4, 256), np.uint8)
        if self.o.orc_fx_luts(kind, pal, prm[0], prm[1], prm[2], luts.ctypes.data) != ps:
            raise Refused("orc_fx_luts")
        self.o.orc_byte_luts(P(src), src.strides[0], P(dst), dst.strides[0], w, h, ps, luts.ctypes.data)

    def triple_split(self, s1, s2, dst, w, h, is_bgr, start, sym, end, vert, bw, bc):
        bc = np.array(bc, np.int32)
        self.o.orc_triple_split(P(s1), s1.strides[0], P(s2), s2.strides[0], P(dst), dst.strides[0], w, h, is_bgr, start, sym, end, vert, bw, bc.ctypes.data)

    def composite(self, dst, ow, oh, ps, layers, bg, is_bgr, revz):
        n = len(layers)
        L = (po.CompLayer * max(1, n))()
        for z, (a, w, h, ox, oy, al) in enumerate(layers):
            L[z].src, L[z].irow = a.ctypes.data, a.strides[0]
            L[z].width, L[z].height, L[z].offs_x, L[z].offs_y, L[z].alpha = w, h, ox, oy, al
        self.o.orc_composite(P(dst), dst.strides[0], ow, oh, ps, is_bgr, (ci * 3)(*bg), L, n, revz)

    def blurzoom_seq(self, w, h, pal, mode, pattern, srcs, dsts):
        z = self.o.orc_blurzoom_new(w, h, pal)
        try:
            for a, d in zip(srcs, dsts):
                _rc(self.o.orc_blurzoom_process(z, P(a), a.strides[0], P(d), d.strides[0], mode, pattern), "orc_blurzoom_process")
        finally:
            self.o.orc_blurzoom_free(z)

    def rgbdelay_seq(self, w, h, pal, clamped, plan, srcs, dsts):
        s = self.o.orc_rgbdelay_new()
        try:
            for a, d, (maxcache, on, st) in zip(srcs, dsts, plan):
                _rc(self.o.orc_rgbdelay_process(s, P(a), a.strides[0], P(d), d.strides[0], w, h, pal, clamped, maxcache, on.ctypes.data, st.ctypes.data), "orc_rgbdelay_process")
        finally:
            self.o.orc_rgbdelay_free(s)

    def get_resizable(self, p, hint, cl, up):
        io = (ci * 5)(p, hint, cl, up, 0)
        r = self.o.orc_get_resizable(io)
        return [r] + (list(io) if r == 1 else [0] * 5)

    def planner(self, a, b):
        return [self.o.orc_get_tgt_gamma(a, b), self.o.orc_can_inline_gamma(a, b), self.o.orc_pconv_can_inplace(a, b)]


class GpuSubject:
    """lives_amd.ops on cuda:0: inputs are uploaded, results downloaded into the arrays the family handed over"""
    name = "gpu"

    def __init__(self):
        import torch
        from lives_amd import lib, ops
        self.torch, self.ops, self.lib = torch, ops, lib
        ops.init(0)
        self.L = lib.load()
        self.L.lives_gpu_get_resizable.argtypes = [ctypes.POINTER(ci)] * 5 + [ci]

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def down(self, t, a):
        self.torch.cuda.synchronize()
        a[:] = t.cpu().numpy()

    def pair(self, src, dst):
        """device tensors of a source and a destination that may be the same array (in place)"""
        d = self.up(dst)
        return (d if src is dst else self.up(src)), d

    def run(self, fn, *a, **k):
        try:
            return fn(*a, **k)
        except self.lib.LgpuError as e:
            raise Refused(str(e)[:160])

    def swizzle(self, op, src, dst, w, h, lut):
        s, d = self.pair(src, dst)
        self.run(self.ops.swizzle, op, s, d, w, h, alpha_first=0, lut=lut)
        self.down(d, dst)

    def k2(self, Y, U, V, dst, w, h, opsz, is422, which, q, lut16=None):
        d = self.up(dst)
        if lut16 is not None:
            self.run(self.ops.yuv420p_to_rgb_lut16, self.up(Y), self.up(U), self.up(V), d, w, h, self.up(lut16.view(np.int16)), opsize=opsz, is_422=is422, which_tables=which, pb_quality=q)
        else:
            self.run(self.ops.yuv420p_to_rgb, self.up(Y), self.up(U), self.up(V), d, w, h, opsize=opsz, is_422=is422, which_tables=which, pb_quality=q)
        self.down(d, dst)

    def gamma_apply(self, pix, x, y, rw, rh, ps, af, lut):
        d = self.up(pix)
        self.run(self.ops.gamma_apply, d, rw, rh, ps, lut, alpha_first=af, x=x, y=y)
        self.down(d, pix)

    def gamma_lut8(self, fileg, f, t, sg):
        lut = np.zeros(256, np.uint8)
        return self.L.lgpu_gamma_lut8(cd(fileg), f, t, cd(sg), P(lut)), lut

    def gamma_lut16(self, fileg, f, t, sg):
        lut = np.zeros(65536, np.uint16)
        return self.L.lgpu_gamma_lut16(cd(fileg), f, t, cd(sg), P(lut)), lut

    def rgb_to_yuv(self, src, planes, w, h, in_order, in_alpha, out_fmt, out_alpha, which):
        d = [self.up(a) for a in planes]
        self.run(self.ops.rgb_to_yuv, self.up(src), d, w, h, in_order, in_alpha, out_fmt, out_alpha, which)
        for t, a in zip(d, planes):
            self.down(t, a)

    def rgb_to_yuv_lut16(self, src, dst, w, h, order, alpha, fmt, unc, lut):
        d = self.up(dst)
        self.run(self.ops.rgb_to_yuv_lut16, self.up(src), d, w, h, order, alpha, fmt, unc, self.up(lut.view(np.int16)))
        self.down(d, dst)

    def yuv_to_rgb(self, planes, dst, w, h, in_fmt, in_alpha, out_order, out_alpha, which):
        d = self.up(dst)
        self.run(self.ops.yuv_to_rgb, [self.up(a) for a in planes], d, w, h, in_fmt, in_alpha, out_order, out_alpha, which)
        self.down(d, dst)

    def yuv_repack(self, ip, op, src, dst, w, h, unc, sampling):
        d = [self.up(a) for a in dst]
        self.run(self.ops.yuv_repack, ip, op, [self.up(a) for a in src], d, w, h, unc, sampling)
        for t, a in zip(d, dst):
            self.down(t, a)

    def yuv411_to_rgb(self, src, wm, h, dst, order, oa, uncl):
        d = self.up(dst)
        self.run(self.ops.yuv411_to_rgb, self.up(src), d, wm, h, out_order=order, out_alpha=oa, unclamped=uncl)
        self.down(d, dst)

    def rgb_to_yuv411(self, src, w, h, order, ia, dst, uncl):
        d = self.up(dst)
        self.run(self.ops.rgb_to_yuv411, self.up(src), d, w, h, in_order=order, in_alpha=ia, unclamped=uncl)
        self.down(d, dst)

    def yuv_yuv_tables(self):
        """a 0..255 ramp through lgpu_yuv_switch_clamping: Y and chroma plane, both directions"""
        out = {}
        ramp = np.arange(256, dtype=np.uint8).reshape(1, 256)
        for to_uncl in (1, 0):
            planes = [self.up(ramp) for _ in range(3)]
            self.run(self.ops.yuv_switch_clamping, planes, 544, 1, to_uncl)
            self.torch.cuda.synchronize()
            out[to_uncl] = (planes[0].cpu().numpy()[0], planes[1].cpu().numpy()[0])
        return [out[1][0], out[1][1], out[0][0], out[0][1]]

    def premult_yuv_tables(self):
        t = [np.zeros((256, 256), np.uint8) for _ in range(4)]
        self.L.lgpu_premult_yuv_tables(*[P(x) for x in t])
        return t

    def _two(self, fn, s1, s2, dst, *a, **k):
        pre = k.pop("pre", ())
        d1, d = self.pair(s1, dst)
        self.run(fn, *pre, d1, self.up(s2), d, *a, **k)
        self.down(d, dst)

    def blend_chroma(self, s1, s2, dst, w, h, ps, af, bf):
        self._two(self.ops.blend_chroma, s1, s2, dst, w, h, ps, bf, alpha_first=af)

    def blend_luma(self, kind, s1, s2, dst, w, h, ps, order, thr):
        self._two(self.ops.blend_luma, s1, s2, dst, w, h, ps, order, thr, pre=(kind,))

    def blend_multi(self, kind, s1, s2, dst, w, h, is_bgr, bf):
        self._two(self.ops.blend_multi, s1, s2, dst, w, h, is_bgr, bf, pre=(kind,))

    def colorkey(self, s0, s1, dst, w, h, is_bgr, delta, opac, col):
        self._two(self.ops.colorkey, s0, s1, dst, w, h, is_bgr, delta, opac, col)

    def mirror(self, mode, src, dst, w, h, ps):
        s, d = self.pair(src, dst)
        self.run(self.ops.mirror, mode, s, d, w, h, ps)
        self.down(d, dst)

    def softlight(self, src, dst, w, h, pal, unc):
        d = [self.up(a) for a in dst]
        self.run(self.ops.softlight, [self.up(a) for a in src], d, w, h, pal, unc)
        for t, a in zip(d, dst):
            self.down(t, a)

    def edge(self, src, dst, w, h, pal, mode):
        s, d = self.pair(src, dst)
        self.run(self.ops.edge, s, d, w, h, pal, mode)
        self.down(d, dst)

    def transition(self, t, s1, s2, dst, w, h, ps, amt):
        self._two(self.ops.transition, s1, s2, dst, w, h, ps, amt, pre=(t,))

    def dissolve(self, s1, s2, dst, w, h, ps, seed, amt):
        dm = self.torch.from_numpy(self.ops.dissolve_mask(seed, w, h)).cuda()
        self._two(self.ops.dissolve, s1, s2, dst, w, h, ps, dm, amt)

    def slide_over(self, s1, s2, dst, w, h, ps, tv, dirn, mvl, mvu):
        self._two(self.ops.slide_over, s1, s2, dst, w, h, ps, tv, dirn, mvl, mvu)

    def deinterlace(self, src, dst, w, h, pal):
        s, d = self.pair(src, dst)
        self.run(self.ops.deinterlace, s, d, w, h, pal)
        self.down(d, dst)

    def script_fx(self, kind, pal, prm, src, dst, w, h, ps):
        luts = self.ops.fx_luts(kind, pal, prm[0], prm[1], prm[2])
        if luts is None or luts.shape[0] != ps:
            raise Refused("lgpu_fx_luts")
        s, d = self.pair(src, dst)
        self.run(self.ops.byte_luts, s, d, w, h, ps, luts)
        self.down(d, dst)

    def triple_split(self, s1, s2, dst, w, h, is_bgr, start, sym, end, vert, bw, bc):
        self._two(self.ops.triple_split, s1, s2, dst, w, h, is_bgr, start, sym, end, vert, bw, bc)

    def composite(self, dst, ow, oh, ps, layers, bg, is_bgr, revz):
        d = self.up(dst)
        self.run(self.ops.composite, d, ow, oh, ps, [(self.up(a), w, h, ox, oy, al) for (a, w, h, ox, oy, al) in layers], bgcol=bg, is_bgr=is_bgr, revz=revz)
        self.down(d, dst)

    def blurzoom_seq(self, w, h, pal, mode, pattern, srcs, dsts):
        g = self.run(self.ops.Blurzoom, w, h, pal)
        try:
            for a, dd in zip(srcs, dsts):
                d = self.up(dd)
                self.run(g.process, self.up(a), d, mode, pattern)
                self.down(d, dd)
        finally:
            g.close()

    def rgbdelay_seq(self, w, h, pal, clamped, plan, srcs, dsts):
        g = self.run(self.ops.RgbDelay)
        try:
            for a, dd, (maxcache, on, st) in zip(srcs, dsts, plan):
                s, d = self.pair(a, dd)
                self.run(g.process, s, d, w, h, pal, maxcache, on, st, yuv_clamped=bool(clamped))
                self.down(d, dd)
        finally:
            g.close()

    def get_resizable(self, p, hint, cl, up):
        pal, xpal, ocl, opal, xopal = (ci(v) for v in (p, 0, cl, hint, 0))
        r = self.L.lives_gpu_get_resizable(ctypes.byref(pal), ctypes.byref(xpal), ctypes.byref(ocl), ctypes.byref(opal), ctypes.byref(xopal), up)
        return [r] + ([pal.value, xpal.value, ocl.value, opal.value, xopal.value] if r == 1 else [0] * 5)

    def planner(self, a, b):
        return [self.L.lives_gpu_get_tgt_gamma(a, b), None, None]      # can_inline_gamma / pconv_can_inplace answer for the library's own bodies (include/lives_gpu_layer.h)


# ---- the reference side -------------------------------------------------------------------------------------------------------------------
class Ref:
    def __init__(self):
        self.R = po.csref()
        self.H = po.RefHost()
        R = self.R
        R.csref_k1.argtypes = [ci, vp, ci, ci, ci, ci, vp, vp, ci]
        R.csref_yuv420p_to_rgb.argtypes = [vp, vp, vp, ci, ci, vp, ci, vp, ci, ci, ci, ci, vp]
        R.csref_gamma_apply.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp]
        R.csref_k4_lut16.argtypes = [ci, ci, vp, ci, ci, ci, ci, vp, ci, ci, vp]
        R.csref_yuv411_to_rgb.argtypes = [vp, ci, ci, vp, ci, ci, ci, ci]
        R.csref_rgb_to_yuv411.argtypes = [vp, ci, ci, ci, ci, ci, vp, ci]
        R.csref_unal_yuv.argtypes = [vp] * 4
        self.C = ctypes.CDLL(os.path.join(po.REFDIR, "libcompref.so"))
        self.C.compref_paint_layer.argtypes = [vp, ci, ci, ci, ci, vp, ci, ci, ci, ci, ci, cd]
        self.Z = ctypes.CDLL(os.path.join(po.REFDIR, "libresizableref.so"))
        self.tmp = tempfile.mkdtemp(prefix="fuzz_oracle_")
        self.private = os.path.join(self.tmp, "libcsref_private.so")
        shutil.copy(os.path.join(po.REFDIR, "libcsref.so"), self.private)
        self.prefs(2, 1, 1.4)
        self._lut16 = {}

    def close(self):
        shutil.rmtree(self.tmp, ignore_errors=True)

    def prefs(self, q, nthr, sg):
        self.R.csref_set_prefs(q, nthr, sg)

    def fresh_lut(self, bits, fileg, f, t, sg):
        """create_gamma_lut8 / create_gamma_lut cache under the wrong key: every table comes from a freshly loaded private copy of the
        slice library, unloaded again afterwards"""
        import _ctypes
        lib = ctypes.CDLL(self.private)
        try:
            lib.csref_set_prefs.argtypes = [ci, ci, cd]
            lib.csref_set_prefs(2, 1, sg)
            out = np.zeros(256 if bits == 8 else 65536, np.uint8 if bits == 8 else np.uint16)
            fn = lib.csref_gamma_lut8 if bits == 8 else lib.csref_gamma_lut16
            fn.argtypes = [cd, ci, ci, vp]
            with quiet_stderr():
                ok = fn(fileg, f, t, P(out))
        finally:
            _ctypes.dlclose(lib._handle)
        return ok, out

    def lut16(self, name):
        if name not in self._lut16:
            f, t = map(int, name.split("_"))
            ok, lut = self.fresh_lut(16, 1.0, f, t, 1.4)
            assert ok == 1
            self._lut16[name] = lut
        return self._lut16[name]


# ---- comparison ---------------------------------------------------------------------------------------------------------------------------
class Mismatch(Exception):
    pass


def same(got, want, what, mask=None):
    """whole arrays, padding included; mask: 1 where the reference's bytes are defined"""
    assert got.shape == want.shape, (got.shape, want.shape)
    d = got != want
    if mask is not None:
        d &= mask.astype(bool)
    if d.any():
        idx = np.argwhere(d)[0]
        raise Mismatch("%s: %d bytes differ, first at %s subject %d reference %d" % (what, int(d.sum()), idx.tolist(), int(got[tuple(idx)]), int(want[tuple(idx)])))


class Ctx:
    """what a family function gets: the random stream, the reference, the subject and the mask ledger"""

    def __init__(self, rng, ref, subj, geometry=None):
        self.rng, self.ref, self.S, self.d = rng, ref, subj, Draw(rng, geometry)
        self.masked_bytes = 0
        self.overmasked = 0
        self.redrawn = 0

    def note_mask(self, mask, allowed, what):
        n = int(mask.size - np.count_nonzero(mask))
        self.masked_bytes += n
        if n > allowed:
            self.overmasked += 1
            raise Mismatch("%s: the mask covers %d bytes, the manifest describes at most %d" % (what, n, allowed))


def draw_case(family, fn, x):
    for _ in range(1000):
        c = fn()
        if not excluded(family, c):
            return c
        x.redrawn += 1
    raise RuntimeError("no admissible draw for " + family)


# ---- families -----------------------------------------------------------------------------------------------------------------------------
def fam_k1(x):
    d = x.d

    def mk():
        name, inplace, nthr = K1_CANON[d.i(0, len(K1_CANON))]
        w, h = d.wh("swizzle")
        return dict(op=name, inplace=inplace, nthr=nthr, w=w, h=h, lut=(name == "delpre") or x.rng.random() < 0.5)
    c = draw_case("k1", mk, x)
    op = po.OPS.index(c["op"])
    ib, ob, w, h = po.OP_IBPP[op], po.OP_OBPP[op], c["w"], c["h"]
    lut = x.rng.integers(0, 256, 256, dtype=np.uint8) if c["lut"] else None
    src = d.fr(w, h, ib)
    x.ref.prefs(2, c["nthr"], 1.4)
    try:
        if c["inplace"]:
            want = gcopy(src)
            x.ref.R.csref_k1(op, P(want), w, h, want.strides[0], want.strides[0], P(want), P(lut), 0)
            got = gcopy(src)
        else:
            init = guarded((h, (w * ob + 3) // 4 * 4 + d.i(0, 3) * 4), fill=0xAB)
            want, got = gcopy(init), gcopy(init)
            x.ref.R.csref_k1(op, P(gcopy(src)), w, h, src.strides[0], want.strides[0], P(want), P(lut), 0)
    finally:
        x.ref.prefs(2, 1, 1.4)
    x.S.swizzle(op, src, got, w, h, lut)
    same(got, want, "k1 %s" % c)


def k2_ref_pixels(buf, w, h, which, opsz, is422, orow):
    """the reference's frame as [h, w, opsz] out of a buffer with one spare row in front: unclamped 4:2:0 rows 1..h-2 start one byte early (K2-f)"""
    flat = buf.reshape(-1)
    out = np.zeros((h, w, opsz), np.uint8)
    for i in range(h):
        shift = 1 if ((which & 1) and not is422 and 1 <= i <= h - 2) else 0
        start = (i + 1) * orow - shift
        out[i] = flat[start:start + w * opsz].reshape(w, opsz)
    return out


def _k2(x, family, lut16):
    d = x.d

    def mk():
        wp, h = d.wh("k2")
        return dict(w=2 * wp, h=h, is422=d.i(0, 2), opsz=int(x.rng.choice([3, 4])), which=d.i(0, 4), q=int(x.rng.choice([1, 2, 3])), pad=8 * d.i(0, 3))
    c = draw_case(family, mk, x)
    w, h, is422, opsz, which, q = c["w"], c["h"], c["is422"], c["opsz"], c["which"], c["q"]
    ys = (w + 7) // 8 * 8 + c["pad"]
    cs = ys // 2
    ch = h if is422 else (h + 1) // 2
    Y = guarded((h, ys), rng=x.rng)
    # the reference reads one sample past each chroma plane on the last pair: the guard byte behind the plane repeats the last sample
    Ub, Vb = (guarded((1, ch * cs + 1), rng=x.rng) for _ in range(2))
    Ub[0, -1], Vb[0, -1] = Ub[0, -2], Vb[0, -2]
    U, V = Ub[0, :-1].reshape(ch, cs), Vb[0, :-1].reshape(ch, cs)
    orow = (w * opsz + 15) // 16 * 16
    buf = guarded((h + 2, orow), fill=0xAB)
    got = guarded((h, orow), fill=0xAB)
    st = (ci * 3)(ys, cs, cs)
    x.ref.prefs(q, 1, 1.4)
    try:
        x.ref.R.csref_yuv420p_to_rgb(P(Y), P(U), P(V), w, h, st, orow, vp(buf.ctypes.data + orow), int(opsz == 4), is422, which & 1, 2 if which & 2 else 1, P(lut16))
    finally:
        x.ref.prefs(2, 1, 1.4)
    x.S.k2(Y, U, V, got, w, h, opsz, is422, which, q, lut16=lut16)
    want = k2_ref_pixels(buf, w, h, which, opsz, is422, orow)
    mask = np.ones((h, w), np.uint8)
    allowed = 0
    if masked(family, c):
        mask[0, 1::2] = 0
        allowed = w // 2
        if h % 2 == 0:
            mask[h - 1, 1::2] = 0
            allowed += w // 2
        if which & 1:
            mask[:, w - 1] = 0
            mask[0, :] = 0
            mask[h - 1, :] = 0
            if h > 1:
                mask[1, 0] = 0
            allowed = 2 * w + h + 1
        x.note_mask(mask, allowed, "%s %s" % (family, c))
    gp = got[:, :w * opsz].reshape(h, w, opsz)
    diff = (gp != want).any(axis=2) & mask.astype(bool)
    if diff.any():
        raise Mismatch("%s %s: %d pixels differ, first %s" % (family, c, int(diff.sum()), np.argwhere(diff)[0].tolist()))
    if not (got[:, w * opsz:] == 0xAB).all():
        raise Mismatch("%s %s: the subject wrote into the row padding" % (family, c))


def fam_k2(x):
    _k2(x, "k2", None)


def fam_k2_lut16(x):
    _k2(x, "k2_lut16", x.ref.lut16("-1_1"))


def fam_k6(x):
    d = x.d
    ps = int(x.rng.choice([3, 4]))
    w, h = d.wh("gamma")
    sx, sy = d.i(0, w), d.i(0, h)
    rw, rh = d.i(1, w - sx + 1), d.i(1, h - sy + 1)
    af = d.i(0, 2) if ps == 4 else 0
    lut = x.rng.integers(0, 256, 256, dtype=np.uint8)
    pix = d.fr(w, h, ps)
    want, got = gcopy(pix), gcopy(pix)
    x.ref.R.csref_gamma_apply(vp(want.ctypes.data + sy * want.strides[0]), rw, rh, want.strides[0], ps, af, sx, P(lut))
    x.S.gamma_apply(got, sx, sy, rw, rh, ps, af, lut)
    same(got, want, "k6 %dx%d ps=%d sub=(%d,%d,%d,%d) af=%d stride=%d" % (w, h, ps, sx, sy, rw, rh, af, pix.strides[0]))


def _lut(x, bits):
    d = x.d
    sg = 1.4 if x.rng.random() < 0.7 else float(x.rng.uniform(1.0, 2.6))
    if x.rng.random() < 0.6:
        fileg, f, t = 1.0, GAMMA_IDS[d.i(0, 4)], GAMMA_IDS[d.i(0, 4)]
    else:                                       # a file gamma on the way to WEED_GAMMA_VARIANT (2048), as oracle/ref/gen_golden.py draws it
        fileg, f, t = float(x.rng.choice([2.2, 0.45, float(x.rng.uniform(0.3, 3.0))])), GAMMA_IDS[d.i(0, 4)], 2048
    ok, want = x.ref.fresh_lut(bits, fileg, f, t, sg)
    gok, got = (x.S.gamma_lut8 if bits == 8 else x.S.gamma_lut16)(fileg, f, t, sg)
    what = "gamma_lut%d fileg=%r from=%d to=%d screen_gamma=%r" % (bits, fileg, f, t, sg)
    if bool(ok) != bool(gok):
        raise Mismatch("%s: reference returned %d, subject %d" % (what, ok, gok))
    if ok:
        same(got.reshape(1, -1), want.reshape(1, -1), what)


def fam_gamma_lut8(x):
    _lut(x, 8)


def fam_gamma_lut16(x):
    _lut(x, 16)


def fam_k4(x):
    d = x.d

    def mk():
        in_order, out_fmt = d.i(0, 3), d.i(0, 6)
        w, h = d.wh("rgb2yuv")
        if out_fmt >= 2:
            w = 2 * max(1, w // 2)
        if out_fmt == 4:
            h = 2 * max(1, h // 2)
        return dict(in_order=in_order, out_fmt=out_fmt, in_alpha=1 if in_order == 2 else d.i(0, 2), out_alpha=d.i(0, 2) if out_fmt <= 1 else 0,
                    which=d.i(0, 4) if out_fmt >= 4 else d.i(0, 2), w=w, h=h, compact=True if out_fmt >= 2 else bool(d.i(0, 2)))
    c = draw_case("k4", mk, x)
    w, h = c["w"], c["h"]
    src = d.fr(w, h, 4 if c["in_alpha"] else 3)
    init, _dims = po.k4_out_planes(0x5A, w, h, c["out_fmt"], c["out_alpha"], compact=c["compact"])
    want, got = [gcopy(a) for a in init], [gcopy(a) for a in init]
    wp, ws = po.planes_args(want)
    r = x.ref.R.csref_k4(c["in_order"], c["in_alpha"], c["out_fmt"], c["out_alpha"], P(src), src.strides[0], w, h, ctypes.addressof(wp), ctypes.addressof(ws), c["which"] & 1, c["which"] >> 1)
    if r != 0:
        raise Mismatch("k4 %s: the reference returned %d" % (c, r))
    x.S.rgb_to_yuv(src, got, w, h, c["in_order"], c["in_alpha"], c["out_fmt"], c["out_alpha"], c["which"])
    for i in range(len(want)):
        same(got[i], want[i], "k4 %s stride=%d plane %d" % (c, src.strides[0], i))


def fam_k4_lut16(x):
    d = x.d
    order = d.i(0, 3)
    alpha = 1 if order == 2 else d.i(0, 2)
    fmt, unc = d.i(2, 4), d.i(0, 2)
    lname = ["-1_1", "1_-1", "1_2"][d.i(0, 3)]
    w, h = d.wh("rgb2yuv")
    w = 2 * max(1, w // 2)
    src = d.fr(w, h, 4 if alpha else 3)
    want, got = guarded((h, w * 2), fill=0x5A), guarded((h, w * 2), fill=0x5A)        # compact destination (K4-c)
    lut = x.ref.lut16(lname)
    what = "k4_lut16 lut=%s order=%d alpha=%d fmt=%d unc=%d %dx%d stride=%d" % (lname, order, alpha, fmt, unc, w, h, src.strides[0])
    r = x.ref.R.csref_k4_lut16(order, alpha, P(src), w, h, src.strides[0], fmt, P(want), want.strides[0], unc, P(lut))
    if r != 0:
        raise Mismatch("%s: the reference returned %d" % (what, r))
    x.S.rgb_to_yuv_lut16(src, got, w, h, order, alpha, fmt, unc, lut)
    # K4-g: the bytes whose LUT index the reference takes from outside 0 .. 65535, worked out from its own tables
    t9, t5 = np.zeros((9, 256), np.int32), np.zeros((5, 256), np.int32)
    x.ref.R.csref_tables(unc, P(t9), P(t5))
    px = src[:, :w * (4 if alpha else 3)].reshape(h, w, 4 if alpha else 3).astype(np.intp)
    ro, go, bo = ((0, 1, 2), (2, 1, 0), (1, 2, 3))[order]
    r, g, b = px[..., ro], px[..., go], px[..., bo]
    idx = lambda k, sel: ((t9[k][r[:, sel]].astype(np.int64) + t9[k + 1][g[:, sel]] + t9[k + 2][b[:, sel]]) >> 8)
    bad = lambda i: (i < 0) | (i > 65535)
    mask = np.ones((h, w * 2), np.uint8)
    ypos, upos, vpos = ((1, 0, 2) if fmt == 2 else (0, 1, 3))
    mask[:, ypos::4][bad(idx(0, slice(0, None, 2)))] = 0
    mask[:, ypos + 2::4][bad(idx(0, slice(1, None, 2)))] = 0
    mask[:, upos::4][bad(idx(3, slice(0, None, 2)))] = 0
    mask[:, vpos::4][bad(idx(6, slice(1, None, 2)))] = 0
    if not (mask[:, ypos::2] == 1).all():
        raise Mismatch("%s: a luma index outside the LUT (the exception covers chroma bytes only)" % what)
    x.note_mask(mask, w * h, what)               # chroma bytes only: half of the destination at the very most
    same(got, want, what, mask=mask)


def fam_k3(x):
    d = x.d

    def mk():
        in_fmt, out_order = d.i(0, 4), d.i(0, 3)
        w, h = d.wh("yuv2rgb")
        if in_fmt >= 2:
            w = 2 * max(1, w // 2)
        return dict(in_fmt=in_fmt, out_order=out_order, in_alpha=d.i(0, 2) if in_fmt <= 1 else 0, out_alpha=1 if out_order == 2 else d.i(0, 2),
                    which=d.i(0, 4) if in_fmt == 0 else d.i(0, 2), w=w, h=h, stride=d.stride(w, 2) if in_fmt >= 2 else 0)
    c = draw_case("k3", mk, x)
    w, h = c["w"], c["h"]
    if c["in_fmt"] == 0:
        planes = [d.fr(w, h, 4 if c["in_alpha"] else 3)]
    elif c["in_fmt"] == 1:
        st = d.stride(w, 1, extra=0)
        planes = [d.fr(w, h, 1, stride=st) for _ in range(4 if c["in_alpha"] else 3)]
    else:
        planes = [d.fr(w, h, 2, stride=c["stride"])]
    opsz = 4 if (c["out_order"] == 2 or c["out_alpha"]) else 3
    want = guarded((h, (w * opsz + 31) // 32 * 32), fill=0x5A)
    got = gcopy(want)
    sp, ss = po.planes_args(planes)
    r = x.ref.R.csref_k3(c["in_fmt"], c["in_alpha"], c["out_order"], c["out_alpha"], ctypes.addressof(sp), ctypes.addressof(ss), w, h, P(want), want.strides[0], c["which"] & 1, c["which"] >> 1)
    if r != 0:
        raise Mismatch("k3 %s: the reference returned %d" % (c, r))
    x.S.yuv_to_rgb(planes, got, w, h, c["in_fmt"], c["in_alpha"], c["out_order"], c["out_alpha"], c["which"])
    same(got, want, "k3 %s stride=%d" % (c, planes[0].strides[0]))


def _planes(pal, w, h, rng=None, fill=0x5A, pad=0):
    return [gcopy(a) for a in po.yuv_planes(pal, w, h, rng=rng, fill=fill, pad=pad)]


def _repack(x, family, c, sampling=0, mask_fn=None):
    ip, op, w, h, unc, pad = c["ip"], c["op"], c["w"], c["h"], c["unc"], c["pad"]
    src = _planes(ip, w, h, rng=x.rng, pad=pad)
    oh = h + ((h & 1) if (family == "repack411" and op in (512, 513)) else 0)
    want = _planes(op, w, oh, pad=0 if family == "repack411" else pad)
    got = [gcopy(a) for a in want]
    sp, ss = po.planes_args(src)
    wp, ws = po.planes_args(want)
    what = "%s %s sampling=%d" % (family, c, sampling)
    r = x.ref.R.csref_yuv_repack(ip, op, ctypes.addressof(sp), ctypes.addressof(ss), ctypes.addressof(wp), ctypes.addressof(ws), w, h, unc, sampling)
    if r != 0:
        raise Mismatch("%s: the reference returned %d" % (what, r))
    x.S.yuv_repack(ip, op, src, got, w, h, unc, sampling)
    for i in range(len(want)):
        same(got[i], want[i], "%s plane %d" % (what, i), mask=mask_fn(want[i].shape) if (mask_fn and i == 0) else None)


def fam_repack(x):
    d = x.d

    def mk():
        ip, op, padok = po.YUV_REPACK_PAIRS[d.i(0, len(po.YUV_REPACK_PAIRS))]
        wp, hp = d.wh("repack")
        return dict(ip=ip, op=op, w=2 * wp, h=2 * hp, pad=int(x.rng.choice([0, 4, 24])) if padok else 0, unc=d.i(0, 2))
    _repack(x, "repack", draw_case("repack", mk, x))


def fam_repack411(x):
    d = x.d
    ip, op, padok = po.YUV411_REPACK_PAIRS[d.i(0, len(po.YUV411_REPACK_PAIRS))]
    wq, h = d.wh("repack411")
    if ip in (512, 513):
        h += h & 1
    _repack(x, "repack411", dict(ip=ip, op=op, w=4 * wq, h=h, pad=int(x.rng.choice([0, 4, 24])) if padok else 0, unc=d.i(0, 2)))


def fam_chroma_up(x):
    d = x.d
    ip, op = po.CHROMA_UP_PAIRS[d.i(0, len(po.CHROMA_UP_PAIRS))]
    wp, hp = d.wh("repack")
    c = dict(ip=ip, op=op, w=2 * wp, h=2 * hp, pad=int(x.rng.choice([0, 4, 24])), unc=d.i(0, 2))

    def mask_fn(shape):
        m = po.chroma_up_mask(ip, op, c["w"], c["h"], c["pad"], shape)
        if masked("chroma_up", c):
            x.note_mask(m, 2 * (2 if ip in (512, 513) else 1), "chroma_up %s" % c)        # the U and V byte of one pixel per affected row
        elif not m.all():
            raise Mismatch("chroma_up %s: a mask outside the exception table" % c)
        return m
    _repack(x, "chroma_up", c, sampling=d.i(0, 2), mask_fn=mask_fn)


def fam_yuv411_to_rgb(x):
    d = x.d
    wm, h = d.wh("yuv411")
    order, uncl = d.i(0, 3), d.i(0, 2)
    oa = 1 if order == 2 else d.i(0, 2)
    ps = 4 if oa else 3
    src = guarded((h, wm * 6), rng=x.rng)
    init = guarded((h, wm * 4 * ps + d.i(0, 5) * 4), rng=x.rng)
    want, got = gcopy(init), gcopy(init)
    x.ref.R.csref_yuv411_to_rgb(P(src), wm, h, P(want), want.strides[0], order, oa, uncl)
    x.S.yuv411_to_rgb(src, wm, h, got, order, oa, uncl)
    same(got, want, "yuv411_to_rgb %dx%d order=%d alpha=%d unclamped=%d stride=%d" % (wm, h, order, oa, uncl, init.strides[0]))


def fam_rgb_to_yuv411(x):
    d = x.d
    w, h = d.wh("rgb411")
    order, uncl = d.i(0, 3), d.i(0, 2)
    ia = 1 if order == 2 else d.i(0, 2)
    src = guarded((h, w * (4 if ia else 3) + d.i(0, 9)), rng=x.rng)
    want, got = guarded((h, (w >> 2) * 6), fill=0x5A), guarded((h, (w >> 2) * 6), fill=0x5A)
    x.ref.R.csref_rgb_to_yuv411(P(src), src.strides[0], w, h, order, ia, P(want), uncl)
    x.S.rgb_to_yuv411(src, w, h, order, ia, got, uncl)
    same(got, want, "rgb_to_yuv411 %dx%d order=%d alpha=%d unclamped=%d stride=%d" % (w, h, order, ia, uncl, src.strides[0]))


def fam_clamp_tables(x):
    """exhaustive, one table entry per case: init_YUV_to_YUV_tables' four tables, 256 entries each (1,024 cases make one full sweep)"""
    st = x.__dict__.setdefault("_clamp", None)
    if st is None:
        ref = [np.zeros(256, np.uint8) for _ in range(4)]
        x.ref.R.csref_yuv_yuv_tables(*[P(t) for t in ref])
        st = x._clamp = [ref, x.S.yuv_yuv_tables(), 0]
    k = st[2] % 1024
    st[2] += 1
    if st[0][k >> 8][k & 255] != st[1][k >> 8][k & 255]:
        raise Mismatch("clamp_tables: table %d entry %d: subject %d reference %d" % (k >> 8, k & 255, st[1][k >> 8][k & 255], st[0][k >> 8][k & 255]))


def fam_premult_tables(x):
    """exhaustive, one table row (256 entries) per case: init_unal's unalcy / alcy / unalcuv / alcuv (1,024 cases make one full sweep)"""
    st = x.__dict__.setdefault("_premult", None)
    if st is None:
        ref = [np.zeros(65536, np.int32) for _ in range(4)]
        x.ref.R.csref_unal_yuv(*[P(t) for t in ref])
        st = x._premult = [[t.reshape(256, 256) for t in ref], x.S.premult_yuv_tables(), 0]
    k = st[2] % 1024
    st[2] += 1
    if not np.array_equal(st[0][k >> 8][k & 255], st[1][k >> 8][k & 255].astype(np.int32)):
        raise Mismatch("premult_tables: table %d row %d differs" % (k >> 8, k & 255))


def _plugin(x, plugin, fname, pal, w, h, srcs, dst, params):
    try:
        x.ref.H.run(po.refplugin(plugin), fname, pal, w, h, srcs, dst, params)
    except RuntimeError as e:
        raise Mismatch("the reference declined: %s" % e)


def fam_blend_chroma(x):
    d = x.d
    pal = d.i(1, 6)
    ps = 3 if pal <= 2 else 4
    w, h = d.wh("blend")
    bf, inplace = d.i(0, 256), d.i(0, 2)
    s1, s2 = d.fr(w, h, ps, extra=0), d.fr(w, h, ps, extra=32)
    init = gcopy(s1) if inplace else guarded(s1.shape, fill=0x5A)
    want, got = gcopy(init), gcopy(init)
    _plugin(x, "simple_blend", "chroma blend", pal, w, h, [want if inplace else s1, s2], want, [po.p_int(bf)])
    x.S.blend_chroma(got if inplace else s1, s2, got, w, h, ps, int(pal == 5), bf)
    same(got, want, "blend_chroma pal=%d %dx%d bf=%d inplace=%d strides %d/%d" % (pal, w, h, bf, inplace, s1.strides[0], s2.strides[0]))


def fam_blend_luma(x):
    d = x.d

    def mk():
        pal = d.i(1, 5)
        ps = 3 if pal <= 2 else 4
        w, h = d.wh("luma")
        return dict(pal=pal, ps=ps, kind=d.i(1, 5), thr=d.i(0, 256), inplace=d.i(0, 2), w=w, h=h, stride1=d.stride(w, ps), stride2=d.stride(w, ps), subject=x.S.name)
    c = draw_case("blend_luma", mk, x)
    pal, ps, kind, thr, inplace, w, h = c["pal"], c["ps"], c["kind"], c["thr"], c["inplace"], c["w"], c["h"]
    order = 0 if pal in (1, 3) else 1
    s1, s2 = d.fr(w, h, ps, stride=c["stride1"]), d.fr(w, h, ps, stride=c["stride2"])
    init = gcopy(s1) if inplace else guarded(s1.shape, fill=0x5A)
    want, got = gcopy(init), gcopy(init)
    _plugin(x, "simple_blend", LUMA_FN[kind], pal, w, h, [want if inplace else s1, s2], want, [po.p_int(thr)])
    x.S.blend_luma(kind, got if inplace else s1, s2, got, w, h, ps, order, thr)
    same(got, want, "blend_luma kind=%d pal=%d %dx%d thr=%d inplace=%d strides %d/%d" % (kind, pal, w, h, thr, inplace, s1.strides[0], s2.strides[0]))


def fam_blend_multi(x):
    d = x.d
    kind, is_bgr, bf = d.i(0, 7), d.i(0, 2), d.i(0, 256)
    w, h = d.wh("multi")
    s1, s2 = d.fr(w, h, 3), d.fr(w, h, 3)
    want, got = guarded(s1.shape, fill=0x5A), guarded(s1.shape, fill=0x5A)
    _plugin(x, "multi_blends", MULTI_FN[kind], 2 if is_bgr else 1, w, h, [s1, s2], want, [po.p_int(bf)])
    x.S.blend_multi(kind, s1, s2, got, w, h, is_bgr, bf)
    same(got, want, "blend_multi kind=%d bgr=%d bf=%d %dx%d strides %d/%d" % (kind, is_bgr, bf, w, h, s1.strides[0], s2.strides[0]))


def fam_colorkey(x):
    d = x.d
    w, h = d.wh("colorkey")
    is_bgr, delta, opac = d.i(0, 2), float(x.rng.random()), float(x.rng.random())
    col = [int(v) for v in x.rng.integers(0, 256, 3)]
    s0, s1 = d.fr(w, h, 3), d.fr(w, h, 3)
    # frame 0 near the key colour in half of its pixels, so that the window test decides both ways
    near = np.clip(np.tile(np.array(col[::-1] if is_bgr else col, np.int16), w)[None, :] + x.rng.integers(-40, 41, (h, w * 3)), 0, 255).astype(np.uint8)
    s0[:, :w * 3] = np.where(np.repeat(x.rng.random((h, w)) < 0.5, 3, axis=1), near, s0[:, :w * 3])
    want, got = guarded(s0.shape, fill=0x5A), guarded(s0.shape, fill=0x5A)
    _plugin(x, "colorkey", "colorkey", 2 if is_bgr else 1, w, h, [s0, s1], want, [po.p_double(delta), po.p_double(opac), po.p_rgb(*col)])
    x.S.colorkey(s0, s1, got, w, h, is_bgr, delta, opac, col)
    same(got, want, "colorkey %dx%d bgr=%d delta=%r opac=%r col=%s strides %d/%d" % (w, h, is_bgr, delta, opac, col, s0.strides[0], s1.strides[0]))


def fam_mirror(x):
    d = x.d
    c = dict(inplace=1, ps=int(x.rng.choice([3, 4])), mode=d.i(0, 3))
    c["w"], c["h"] = d.wh("mirror")
    w, h, ps, mode = c["w"], c["h"], c["ps"], c["mode"]
    # two spare rows and at least one spare pixel per row take the reference's stray writes (oracle/ref/gen_golden.py)
    s = d.fr(w, h, ps, stride=d.stride(w + 1, ps), rows=h + 2)
    want, got = gcopy(s), gcopy(s)
    _plugin(x, "mirrors", ["mirrorx", "mirrory", "mirrorxy"][mode], 1 if ps == 3 else 3, w, h, [want], want, [])
    x.S.mirror(mode, got, got, w, h, ps)
    mask = np.ones(s.shape, np.uint8)
    allowed = 0
    if mode != 1 and w % 2 == 0:
        mask[:h + 1, w * ps:(w + 1) * ps] = 0
        allowed += (h + 1) * ps
    if mode != 0:
        mask[h, :(w + 1) * ps] = 0
        allowed += (w + 1) * ps
    x.note_mask(mask, allowed, "mirror %s" % c)
    same(got, want, "mirror %s stride=%d" % (c, s.strides[0]), mask=mask)


def fam_softlight(x):
    d = x.d
    pal = int(x.rng.choice([512, 513, 522, 544, 545]))
    wp, hp = d.wh("softlight")
    w, h, unc = 2 * wp, 2 * hp, d.i(0, 2)
    cw = w >> 1 if pal in (512, 513, 522) else w
    ch = h >> 1 if pal in (512, 513) else h
    dims = [(w, h), (cw, ch), (cw, ch)] + ([(w, h)] if pal == 545 else [])
    src = [d.fr(a, b, 1) for (a, b) in dims]
    want, got = [guarded(a.shape, fill=0x5A) for a in src], [guarded(a.shape, fill=0x5A) for a in src]
    try:
        x.ref.H.run_planar(po.refplugin("softlight"), "softlight", pal, w, h, src, want, unc)
    except RuntimeError as e:
        raise Mismatch("the reference declined: %s" % e)
    x.S.softlight(src, got, w, h, pal, unc)
    for i in range(len(dims)):
        same(got[i], want[i], "softlight pal=%d %dx%d unc=%d plane %d stride %d" % (pal, w, h, unc, i, src[i].strides[0]))


def fam_edge(x):
    d = x.d
    pal, mode = d.i(1, 6), d.i(0, 3)
    ps = 3 if pal <= 2 else 4
    w, h = d.wh("edge")
    if x.rng.random() < 0.5 and d.fixed is None:        # whole quads, as fuzz_ops.py draws them (capped at 300 x 120)
        w, h = 4 * d.i(2, 76), d.i(4, 121)
    inplace = d.i(0, 2)
    sfr = d.fr(w, h, ps)
    yy, xx = np.mgrid[0:h, 0:w]
    for c in range(ps):
        sfr[:, c:w * ps:ps] = ((sfr[:, c:w * ps:ps] >> 3) + (96 * ((xx // 9 + yy // 7 + c) % 2)).astype(np.uint8) + 40).astype(np.uint8)
    init = gcopy(sfr) if inplace else guarded(sfr.shape, rng=x.rng)
    want, got = gcopy(init), gcopy(init)
    _plugin(x, "edge", "edge detect", pal, w, h, [want if inplace else sfr], want, [po.p_int(mode)])
    x.S.edge(got if inplace else sfr, got, w, h, pal, mode)
    same(got, want, "edge pal=%d mode=%d %dx%d inplace=%d stride=%d" % (pal, mode, w, h, inplace, sfr.strides[0]))


def fam_transition(x):
    d = x.d
    t, ps = d.i(0, 3), int(x.rng.choice([3, 4]))
    w, h = d.wh("transition")
    amt = float(x.rng.choice([0., 1., float(x.rng.random())]))
    s1, s2 = d.fr(w, h, ps), d.fr(w, h, ps)
    inplace = d.i(0, 2) if t < 2 else 0
    init = gcopy(s1) if inplace else guarded(s1.shape, fill=0x5A)
    want, got = gcopy(init), gcopy(init)
    _plugin(x, "multi_transitions", ["iris rectangle", "iris circle", "4 way split"][t], 1 if ps == 3 else 4, w, h, [want if inplace else s1, s2], want, [po.p_double(amt)])
    x.S.transition(t, got if inplace else s1, s2, got, w, h, ps, amt)
    same(got, want, "transition %d ps=%d %dx%d amount=%r inplace=%d strides %d/%d" % (t, ps, w, h, amt, inplace, s1.strides[0], s2.strides[0]))


def fam_dissolve(x):
    d = x.d
    ps = int(x.rng.choice([3, 4]))
    w, h = d.wh("transition")
    if d.fixed is None:
        w, h = max(1, w - 1), max(1, h - 1)       # tests/test_gpu_parity.py::test_dissolve runs 1x1 too
    amt = float(x.rng.choice([0., 1., float(x.rng.random())]))
    seed = int(x.rng.integers(1, 2 ** 62))
    inplace = d.i(0, 2)
    s1, s2 = d.fr(w, h, ps), d.fr(w, h, ps)
    init = gcopy(s1) if inplace else guarded(s1.shape, fill=0x5A)
    want, got = gcopy(init), gcopy(init)
    x.ref.H.H.refhost_set_random_seed(seed)
    try:
        with quiet_stderr():
            _plugin(x, "multi_transitions", "dissolve", 1 if ps == 3 else 4, w, h, [want if inplace else s1, s2], want, [po.p_double(amt)])
    finally:
        x.ref.H.H.refhost_set_random_seed(0)
    x.S.dissolve(got if inplace else s1, s2, got, w, h, ps, seed, amt)
    same(got, want, "dissolve ps=%d %dx%d amount=%r seed=%d inplace=%d strides %d/%d" % (ps, w, h, amt, seed, inplace, s1.strides[0], s2.strides[0]))


def fam_slide_over(x):
    d = x.d
    ps = int(x.rng.choice([3, 4]))
    w, h = d.wh("slide")
    tv, dirn, mvl, mvu = d.i(0, 256), d.i(1, 5), d.i(0, 2), d.i(0, 2)
    s1, s2 = d.fr(w, h, ps), d.fr(w, h, ps)
    want, got = guarded(s1.shape, fill=0x5A), guarded(s1.shape, fill=0x5A)
    radios = [po.p_bool(False)] + [po.p_bool(dirn == k) for k in (1, 2, 3)] + [po.p_bool(False)]
    _plugin(x, "slide_over", "slide over", 1 if ps == 3 else 4, w, h, [s1, s2], want, [po.p_int(tv)] + radios + [po.p_bool(mvl), po.p_bool(mvu)])
    x.S.slide_over(s1, s2, got, w, h, ps, tv, dirn, mvl, mvu)
    same(got, want, "slide ps=%d %dx%d amount=%d dir=%d lower=%d upper=%d strides %d/%d" % (ps, w, h, tv, dirn, mvl, mvu, s1.strides[0], s2.strides[0]))


def fam_deinterlace(x):
    d = x.d

    def mk():
        pal = int(x.rng.choice([1, 2, 588, 3, 4, 589, 5, 564, 565]))
        ps = 3 if pal in (1, 2, 588) else 4
        w, h = d.wh("deint")
        return dict(pal=pal, ps=ps, w=w, h=h, inplace=d.i(0, 2), stride=max(d.stride(w, ps), (w + 2) // 3 * 3 * ps if x.rng.random() < 0.9 else 0))
    c = draw_case("deinterlace", mk, x)
    pal, ps, w, h, inplace = c["pal"], c["ps"], c["w"], c["h"], c["inplace"]
    src = d.fr(w, h, ps, stride=c["stride"])
    init = gcopy(src) if inplace else guarded(src.shape, fill=0x5A)
    want, got = gcopy(init), gcopy(init)
    _plugin(x, "deinterlace", "deinterlace", pal, w, h, [want if inplace else src], want, [])
    x.S.deinterlace(got if inplace else src, got, w, h, pal)
    same(got, want, "deinterlace %s" % c)


def fam_script_fx(x):
    d = x.d
    kind = d.i(0, 3)
    pal = d.i(1, 5) if kind == 1 else d.i(1, 6)            # posterise offers no ARGB32
    ps = 3 if pal <= 2 else 4
    prm = (0., 0., 0.) if kind == 0 else (float(d.i(1, 9)), 0., 0.) if kind == 1 else tuple(float(v) for v in np.round(x.rng.uniform(0., 5., 3), 3))
    w, h = d.wh("bytelut")
    inplace = d.i(0, 2)
    fn = ["negate", "posterise", "ccorrect"][kind]
    src = d.fr(w, h, ps)
    init = gcopy(src) if inplace else guarded(src.shape, fill=0x5A)
    want, got = gcopy(init), gcopy(init)
    params = [] if kind == 0 else [po.p_int(int(prm[0]))] if kind == 1 else [po.p_double(v) for v in prm]
    _plugin(x, fn, fn, pal, w, h, [want if inplace else src], want, params)
    x.S.script_fx(kind, pal, prm, got if inplace else src, got, w, h, ps)
    same(got, want, "script_fx %s pal=%d %r %dx%d inplace=%d stride=%d" % (fn, pal, prm, w, h, inplace, src.strides[0]))


def fam_triple_split(x):
    d = x.d
    w, h = d.wh("tsplit")
    start, end, bw = float(x.rng.random()), float(x.rng.random()), float(x.rng.random() * 0.5 * (x.rng.random() < 0.7))
    sym, vert, is_bgr, inplace = (int(v) for v in x.rng.integers(0, 2, 4))
    bc = [int(v) for v in x.rng.integers(0, 256, 3)]
    s1, s2 = d.fr(w, h, 3), d.fr(w, h, 3)
    init = gcopy(s1) if inplace else guarded(s1.shape, fill=0x5A)
    want, got = gcopy(init), gcopy(init)
    prm = [po.p_double(start), po.p_bool(sym), po.p_bool(not sym), po.p_double(end), po.p_bool(vert), po.p_double(bw), po.p_rgb(*bc)]
    _plugin(x, "layout_blends", "triple split", 2 if is_bgr else 1, w, h, [want if inplace else s1, s2], want, prm)
    x.S.triple_split(got if inplace else s1, s2, got, w, h, is_bgr, start, sym, end, vert, bw, bc)
    same(got, want, "tsplit %dx%d %r sym=%d %r vert=%d bw=%r bgr=%d col=%s inplace=%d strides %d/%d" % (w, h, start, sym, end, vert, bw, is_bgr, bc, inplace, s1.strides[0], s2.strides[0]))


def fam_compositor(x):
    """compositor.c's paint loop (libcompref.so: compref_paint_layer) with the background and the z order laid out as oracle/ref/gen_golden_comp.py does (:171-189)"""
    d = x.d
    ps, is_bgr, revz = int(x.rng.choice([3, 4])), d.i(0, 2), d.i(0, 2)
    (ow, oh), n = d.geometry(1, 301, 1, 121), d.i(0, 6)
    bg = [int(v) for v in x.rng.integers(0, 256, 3)]
    layers = []
    for z in range(n):
        w, h = d.i(1, ow + 8), d.i(1, oh + 8)
        layers.append((d.fr(w, h, ps), w, h, d.i(0, ow), d.i(0, oh), float(x.rng.choice([0., 0.25, 0.5, 0.7312, 1., float(x.rng.random())]))))
    want = guarded((oh, po.align(ow * ps)), fill=0x5A)
    got = gcopy(want)
    r, b = (2, 0) if is_bgr else (0, 2)
    px = want[:, :ow * ps].reshape(oh, ow, ps)
    px[..., 0], px[..., 1], px[..., 2] = bg[r], bg[1], bg[b]
    if ps == 4:
        px[..., 3] = 255
    for z in (range(n) if revz else range(n - 1, -1, -1)):
        a, w, h, ox, oy, al = layers[z]
        x.ref.C.compref_paint_layer(P(want), want.strides[0], ow, oh, ps, P(a), a.strides[0], w, h, ox, oy, al)
    x.S.composite(got, ow, oh, ps, layers, bg, is_bgr, revz)
    same(got, want, "compositor ps=%d bgr=%d revz=%d %dx%d bg=%s layers=%s" % (ps, is_bgr, revz, ow, oh, bg, [l[1:] for l in layers]))


def fam_get_resizable(x):
    """exhaustive walk, one question per case: get_resizable over palette x hint x direction x clamping (1,020), then get_tgt_gamma / can_inline_gamma /
    pconv_can_inplace over the palette pairs (225)"""
    k = x.__dict__.get("_rs", 0)
    x._rs = k + 1
    k %= 1020 + 225
    Z = x.ref.Z
    if k < 1020:
        p, hint = RS_PALS[k // 68], (RS_PALS + [0, -1])[(k // 4) % 17]
        up, cl = (k >> 1) & 1, k & 1
        io = (ci * 5)(p, hint, cl, up, 0)
        r = Z.rsref_get_resizable(io)
        want = [r] + (list(io) if r == 1 else [0] * 5)
        got = x.S.get_resizable(p, hint, cl, up)
        if x.S.name == "gpu":
            want[0] = 1 if want[0] == 1 else 0            # the reference's LIVES_FATAL (-1) is a plain refusal in the library
        if got != want:
            raise Mismatch("get_resizable pal=%d hint=%d upscale=%d clamping=%d: subject %s reference %s" % (p, hint, up, cl, got, want))
    else:
        a, b = RS_PALS[(k - 1020) // 15], RS_PALS[(k - 1020) % 15]
        want = [Z.rsref_get_tgt_gamma(a, b), Z.rsref_can_inline_gamma(a, b), Z.rsref_pconv_can_inplace(a, b)]
        got = x.S.planner(a, b)
        if any(g is not None and g != w_ for g, w_ in zip(got, want)):
            raise Mismatch("planner queries %d -> %d: subject %s reference %s" % (a, b, got, want))


# ---- stateful families: one instance over a sequence of 5 .. 12 frames ----------------------------------------------------------------
def fam_blurzoom(x):
    d = x.d
    pal, mode, pattern = d.i(3, 5), d.i(0, 4), d.i(0, 4)
    (w, h), n = d.geometry(32, 301, 8, 41), d.i(5, 13)          # blurzoom.c:262-263 takes 32 pixels and up
    stride = po.align(w * 4) if mode in (0, 3) else w * 4          # strobe modes: compact rows (blurzoom.c:391-396)
    srcs = []
    for f in range(n):
        a = guarded((h, stride), rng=x.rng)
        a[:, :w * 4] = (a[:, :w * 4] >> 4) + 40
        x0 = (6 + 6 * f) % max(1, w - 14)
        a[1 + f % 3:5 + f % 3, x0 * 4:(x0 + 14) * 4] = 250
        srcs.append(a)
    want, got = [guarded(a.shape, fill=0x5A) for a in srcs], [guarded(a.shape, fill=0x5A) for a in srcs]
    try:
        x.ref.H.run_seq(po.refplugin("blurzoom"), "blurzoom", pal, w, h, srcs, want, [po.p_int(mode), po.p_int(pattern)])
    except RuntimeError as e:
        raise Mismatch("the reference declined: %s" % e)
    x.S.blurzoom_seq(w, h, pal, mode, pattern, srcs, got)
    for f in range(n):
        same(got[f], want[f], "blurzoom pal=%d mode=%d pattern=%d %dx%d frame %d of %d" % (pal, mode, pattern, w, h, f, n))


def fam_rgbdelay(x):
    d = x.d
    yuv = x.rng.random() < 0.3
    fn, pal = ("YUVdelay", 588) if yuv else ("RGBdelay", d.i(1, 3))
    clamp = d.i(0, 2) if yuv else -1
    (w, h), n = d.geometry(1, 133, 1, 25), d.i(5, 13)
    maxcache, inplace = d.i(1, 21), d.i(0, 2)
    on, st = np.zeros(51 * 3, np.int32), np.ones(51, np.float64)
    for j in set([0] + [d.i(0, min(maxcache + 2, 51)) for _ in range(d.i(0, 4))]):
        on[3 * j:3 * j + 3] = x.rng.integers(0, 2, 3)
        st[j] = float(x.rng.choice([1.0, round(float(x.rng.random()), 3)]))
    params = [po.p_int(maxcache)]
    for j in range(51):
        params += [po.p_bool(on[3 * j]), po.p_bool(on[3 * j + 1]), po.p_bool(on[3 * j + 2]), po.p_double(st[j])]
    stride = d.stride(w, 3)
    frames = [d.fr(w, h, 3, stride=stride) for _ in range(n)]
    init = [gcopy(f) if inplace else guarded(f.shape, fill=0x5A) for f in frames]
    want, got = [gcopy(a) for a in init], [gcopy(a) for a in init]
    x.ref.H.H.refhost_set_yuv_clamping(clamp)
    try:
        x.ref.H.run_seq(po.refplugin("RGBdelay"), fn, pal, w, h, want if inplace else frames, want, params)
    except RuntimeError as e:
        raise Mismatch("the reference declined: %s" % e)
    finally:
        x.ref.H.H.refhost_set_yuv_clamping(-1)
    x.S.rgbdelay_seq(w, h, pal, 1 if clamp == 0 else 0, [(maxcache, on, st)] * n, got if inplace else frames, got)
    for f in range(n):
        same(got[f], want[f], "rgbdelay %s pal=%d clamp=%d cache=%d %dx%d inplace=%d frame %d of %d on=%s" % (fn, pal, clamp, maxcache, w, h, inplace, f, n, np.nonzero(on)[0].tolist()))


FAMILIES = OrderedDict([
    ("k1", fam_k1), ("k2", fam_k2), ("k2_lut16", fam_k2_lut16), ("k6", fam_k6), ("gamma_lut8", fam_gamma_lut8), ("gamma_lut16", fam_gamma_lut16),
    ("k3", fam_k3), ("k4", fam_k4), ("k4_lut16", fam_k4_lut16), ("repack", fam_repack), ("repack411", fam_repack411), ("chroma_up", fam_chroma_up),
    ("yuv411_to_rgb", fam_yuv411_to_rgb), ("rgb_to_yuv411", fam_rgb_to_yuv411), ("clamp_tables", fam_clamp_tables), ("premult_tables", fam_premult_tables),
    ("blend_chroma", fam_blend_chroma), ("blend_luma", fam_blend_luma), ("blend_multi", fam_blend_multi), ("colorkey", fam_colorkey), ("mirror", fam_mirror),
    ("softlight", fam_softlight), ("edge", fam_edge), ("transition", fam_transition), ("dissolve", fam_dissolve), ("slide_over", fam_slide_over),
    ("deinterlace", fam_deinterlace), ("script_fx", fam_script_fx), ("triple_split", fam_triple_split), ("compositor", fam_compositor),
    ("get_resizable", fam_get_resizable), ("blurzoom", fam_blurzoom), ("rgbdelay", fam_rgbdelay),
])
STATEFUL = ("blurzoom", "rgbdelay")
# exhaustive families: a case is one table entry / row / question, walked in order from 0; run() rounds their case count up to whole sweeps of this length, so
# every run, however few cases it asks for, compares every entry at least once
EXHAUSTIVE = {"clamp_tables": 1024, "premult_tables": 1024, "get_resizable": 1020 + 225}


def run(cases, seed, kinds=None, subject="oracle", sequences=None, verbose=True, max_reports=5, per_family=None, geometry=None):
    """-> {family: dict(drawn, redrawn, compared, skipped, mismatching, masked_bytes, overmasked, first)}; redrawn: draws thrown away because a `never`
    entry of EXCEPTIONS held (they are not part of drawn); skipped: draws neither compared nor mismatching (none today); subject: "oracle", "gpu" or a subject object to use again;
    per_family overrides the case count of single families; geometry: a (width, height) every case takes in place of a drawn one (Draw.fixed)"""
    assert po.have_ref(), "oracle/_ref is not built (oracle/ref/build_ref.sh)"
    subj = GpuSubject() if subject == "gpu" else OracleSubject() if subject == "oracle" else subject
    ref = Ref()
    out = OrderedDict()
    try:
        for k, (name, fn) in enumerate(FAMILIES.items()):
            if kinds and name not in kinds:
                continue
            n = (sequences if sequences is not None else max(1, cases // 10)) if name in STATEFUL else cases
            n = (per_family or {}).get(name, n)
            if name in EXHAUSTIVE:
                n = -(-max(n, 1) // EXHAUSTIVE[name]) * EXHAUSTIVE[name]
            x = Ctx(np.random.default_rng([seed, k]), ref, subj, geometry)
            st = dict(drawn=0, redrawn=0, compared=0, skipped=0, mismatching=0, masked_bytes=0, overmasked=0, first=None)
            for _ in range(n):
                st["drawn"] += 1
                try:
                    fn(x)
                    st["compared"] += 1
                except Refused as e:                    # the reference served the draw, the subject did not
                    st["mismatching"] += 1
                    msg = "%s: the subject refused a draw the reference served: %s" % (name, e)
                    st["first"] = st["first"] or msg
                    if verbose and st["mismatching"] <= max_reports:
                        print("MISMATCH", msg, flush=True)
                except Mismatch as e:
                    st["mismatching"] += 1
                    st["first"] = st["first"] or str(e)
                    if verbose and st["mismatching"] <= max_reports:
                        print("MISMATCH", e, flush=True)
            st["masked_bytes"], st["overmasked"], st["redrawn"] = x.masked_bytes, x.overmasked, x.redrawn
            out[name] = st
            if verbose:
                print("%-14s compared %6d  skipped %4d  mismatching %4d  masked bytes %d  redrawn %d" % (name, st["compared"], st["skipped"], st["mismatching"], st["masked_bytes"], st["redrawn"]), flush=True)
    finally:
        ref.close()
    return out


def summary(out, subject, seed):
    return "fuzz_oracle: subject=%s seed=%d families=%d compared=%d skipped=%d mismatching=%d" % (
        subject, seed, len(out), sum(s["compared"] for s in out.values()), sum(s["skipped"] for s in out.values()), sum(s["mismatching"] for s in out.values()))


def parse_summary(line):
    m = re.match(r"fuzz_oracle: subject=(\w+) seed=(\d+) families=(\d+) compared=(\d+) skipped=(\d+) mismatching=(\d+)", line)
    return dict(zip(("subject", "seed", "families", "compared", "skipped", "mismatching"), [m.group(1)] + [int(v) for v in m.groups()[1:]])) if m else None


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    subject = "oracle"
    if "--subject" in argv:
        subject = argv[argv.index("--subject") + 1]
        args.remove(subject)
    cases = int(args[0]) if len(args) > 0 else 200
    seed = int(args[1]) if len(args) > 1 else 1
    kinds = args[2].split(",") if len(args) > 2 else None
    out = run(cases, seed, kinds, subject)
    print(summary(out, subject, seed))
    return 1 if any(s["mismatching"] for s in out.values()) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
