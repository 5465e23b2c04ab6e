"""Every row- and cell-strided kernel on frames taller than its grid cap, bit for bit against the CPU oracle.

About forty-five kernels share one launch shape: grid.y = min(rows, CAP) and `for (y = blockIdx.y; y < rows; y += gridDim.y)`.  The other suites stay below
every cap, so the second trip of those loops (and a trip in which only some blockIdx.y still have a row) runs here and nowhere else.  Frames are narrow
(32 pixels or fewer), so a frame of 8229 rows is a few hundred KB and the oracle takes milliseconds.

CAPS below is the table of launch sites; test_caps_match_the_sources (no GPU) reads lives_amd/csrc/*.hip and fails when a cap changes or a launch site is
added, so the heights here cannot fall behind the code silently.  Heights per site with cap C, in grid units (a unit is a row, or a row pair where the
kernel walks pairs): C + 1 (one blockIdx.y takes a second trip) and 2 C + 37 (three trips, the last one partial); rounded up to even where the operation
needs it.

Which entry point and shape reaches which site:

  swizzle.hip row_grid (4096)        lgpu_swizzle (k_swizzle: 16 pixels on 16-byte aligned rows; k_swizzle_bytes: 13 pixels on odd pitches), lgpu_gamma_apply
                                     (k_gamma_apply / k_gamma_apply_bytes, same two shapes), lgpu_alpha_premult (k_premult<true> / <false>), lgpu_byte_luts
                                     (k_byte_luts<3> / <4>), lgpu_alpha_premult_yuva (k_premult_yuva<1>: clamped YUVA8888 of 16 pixels on aligned rows;
                                     k_premult_yuva<0>: everything else), lgpu_swizzle_batch (three frames: grid.z with the row stride)
  effects.hip row_grid2 (4096)       lgpu_blend_chroma / _luma / _multi / lgpu_colorkey (k_pixel2, vector and byte form), lgpu_blend_chroma with alpha first
                                     (k_chroma_argb), lgpu_mirror (k_mirror_v4: 4-byte pixels on aligned rows; k_mirror<3> / <4>), lgpu_letterbox (k_letterbox<1 / 3 / 4>),
                                     lgpu_letterbox_bars (k_letterbox_bars)
  palette.hip k_clamp_switch (4096 workgroups)   lgpu_yuv_switch_clamping on one 3840x2160 YUVA8888 plane (33 MB against 16.7 MB per pass)
  palette.hip k_rgb_to_yuv (2048)    lgpu_rgb_to_yuv with width & 3 != 0 (18, 22) or 3-byte pixels; the 4:2:0 target walks row pairs; lgpu_rgb_to_yuv_batch
  palette.hip k_yuv_to_rgb (2048)    lgpu_yuv_to_rgb with width & 3 != 0 or 3-byte pixels
  palette.hip k_rgb_to_yuv411 (2048) lgpu_rgb_to_yuv411 (its only kernel)
  palette.hip k_yuv411_repack (2048) lgpu_yuv_repack with palette 595 on either side
  palette.hip k_chroma_up_packed (2048)   lgpu_yuv_repack 4:2:0 / 4:2:2 planar -> YUV888 / YUVA8888
  palette.hip k_yuv_repack (2048)    lgpu_yuv_repack at width 18 (width & 3 != 0 and width & 7 != 0: every `_s` cell form declines); 4:2:0 targets walk row pairs
  palette.hip k_yuv411_to_rgb (8 workgroups per CU)   lgpu_yuv411_to_rgb on one 3840x2160 frame (2,073,600 macropixels)
  yuv.hip k_yuv420p_to_rgb / k_yuv422p_to_rgb (2048)  lgpu_yuv420p_to_rgb with opsize 3, with LOW quality and opsize 4, and lgpu_yuv420p_to_rgb_lut16 (the paired-table
                                     form declines all three); 4:2:0 walks units of a row pair (row 0 and the trailing row are units of their own)
  resize.hip k_hpass_generic / k_vpass_generic (2048) lgpu_resize and lgpu_gauss5 with psize 1 and 3 (gauss5: width & 3 != 0) and psize 4 on a row pitch that is
                                     1 byte off alignment; a tall source strides the h pass, a tall destination the v pass
  effects.hip k_composite / k_slide_over / k_triple_split / k_dissolve (2048)   the entry points of the same names; lgpu_transition (a linear walk without a cap)
                                     rides along because its rules depend on the row
  stencil.hip k_deinterlace (2048 row pairs)   lgpu_deinterlace: heights doubled
  stencil.hip k_edge_paint, k_bz_*, k_rgbdelay, k_rgbdelay4, k_rgbd_snapshot (1024)   lgpu_edge with EDGE_NO_S, lgpu_blurzoom_process, lgpu_rgbdelay_process
                                     (3 * width % 4 != 0: k_rgbdelay; == 0: k_rgbdelay4)
  stencil.hip k_edge_map<PS> (1024 workgroups)   lgpu_edge with EDGE_NO_S on 68 x 8193: 2 x 513 tiles of 64 x 16
  stencil.hip k_edge_map4 (1024 workgroups), k_edge_paint4 (8 workgroups per CU)   lgpu_edge without EDGE_NO_S on 132 x 16385 RGBA: 2 x 513 tiles of 128 x 32 and
                                     540,705 quads against 8 x 256 lanes per CU
  runtime.hip k_fill_pattern (512)   lgpu_fill_pattern.  k_set4 and k_set64 of the same file are single-workgroup launches without a walk, and lgpu_fill is a
                                     hipMemsetAsync; lgpu_fill and lgpu_letterbox_bars are compared with a numpy fill at the same row counts all the same

How a case compares: the output buffer has two guard rows and row padding.  Out of place it starts as the fill byte 0xA5 everywhere, in place as the source with
random padding; the oracle runs on a host copy of the same buffer, and same_whole() asserts that the GPU's buffer equals the oracle's byte for byte -- image, padding
and guard rows at once -- and that the oracle left the guard rows as they were.  That is assert_same + assert_padding_untouched of tests/util.py in one comparison,
and stricter for the two operations whose reference writes its own row padding (rgbdelay zeroes it, the planar 4:4:4 copies carry it over when the pitches agree):
the padding is held to what the oracle -- a plain restatement of the reference, which touches padding in those two places only -- left there, not to the fill.
"""
import collections
import ctypes
import glob
import os
import re
import zlib

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.util import align, dev, frame, host

G = pytest.mark.gpu
P = po.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# launch site (file, kernel or helper) -> cap on grid.y (or on the number of workgroups of a linear walk); one entry per capped launch grid in the sources
CAPS = {
    ("swizzle.hip", "row_grid"): 4096,
    ("effects.hip", "row_grid2"): 4096,
    ("palette.hip", "k_clamp_switch"): 4096,
    ("palette.hip", "k_rgb_to_yuv"): 2048,
    ("palette.hip", "k_yuv_to_rgb"): 2048,
    ("palette.hip", "k_rgb_to_yuv411"): 2048,
    ("palette.hip", "k_yuv411_repack"): 2048,
    ("palette.hip", "k_chroma_up_packed"): 2048,
    ("palette.hip", "k_yuv_repack"): 2048,
    ("yuv.hip", "k_yuv420p_to_rgb"): 2048,              # and k_yuv422p_to_rgb: one grid
    ("resize.hip", "k_hpass_generic/resize"): 2048,
    ("resize.hip", "k_vpass_generic/resize"): 2048,
    ("resize.hip", "k_hpass_generic+k_vpass_generic/gauss5"): 2048,
    ("effects.hip", "k_composite"): 2048,
    ("effects.hip", "k_slide_over"): 2048,
    ("effects.hip", "k_triple_split"): 2048,
    ("effects.hip", "k_dissolve"): 2048,
    ("stencil.hip", "k_deinterlace"): 2048,
    ("stencil.hip", "k_edge_paint"): 1024,
    ("stencil.hip", "k_edge_map"): 1024,
    ("stencil.hip", "k_edge_map4"): 1024,
    ("stencil.hip", "k_bz_update+k_bz_color"): 1024,
    ("stencil.hip", "k_bz_blur+k_bz_zoom"): 1024,
    ("stencil.hip", "k_rgbd_snapshot"): 1024,
    ("stencil.hip", "k_rgbdelay+k_rgbdelay4"): 1024,
    ("runtime.hip", "k_fill_pattern"): 512,
}
# the caps that are no literals: workgroups per CU of a linear walk, with the statement that sets each
PER_CU_CAPS = {("palette.hip", "k_yuv411_to_rgb"): (8, r"\bcap\s*=\s*cdiv\(\(unsigned\)device_cus\(\)\s*\*\s*8u\s*,\s*\(unsigned\)nframes\)"),
               ("stencil.hip", "k_edge_paint4"): (8, r"\bpcap\s*=\s*\(unsigned\)device_cus\(\)\s*\*\s*8u\s*,")}

FILL = 0xA5
GUARD = 2
W = {"v": 16, "b": 13}          # "v": a multiple of 4 pixels on 16-byte aligned rows (the vector forms); "b": 13 pixels on a pitch no vector form takes


def heights(site, unit=1, even=False):
    """the two heights for a launch site: C + 1 and 2 C + 37 grid units of `unit` rows"""
    c = CAPS[site]
    hs = [unit * (c + 1), unit * (2 * c + 37)]
    return [h + (h & 1) for h in hs] if even else hs


def pitch(w, ps, form):
    if form == "v":
        return align(w * ps + 16, 32)
    return w * ps + (4 if ps == 4 else 2)          # 56 (4-byte pixels stay 4-byte aligned, never 16), 41, 15


def seeded(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def flag(h):
    """a setting that differs between the two heights of a site (all of them are C + 1 and 2 C + 37 times a small unit)"""
    return (h >> 2) & 1


def blank(rows, stride):
    return np.full((rows + GUARD, stride), FILL, np.uint8)


def src_frame(rng, w, h, ps, stride):
    return frame(rng, w, h, ps, stride=stride, extra_rows=GUARD)


def guards_kept(want, before, h, what):
    """the oracle left everything past the frame's h rows as it was (needs no device: the runners assert it before they look at `gpu`)"""
    assert (want[h:] == before[h:]).all(), what + ": the oracle wrote past the frame"


def same_whole(got, want, before, h, what):
    """the whole buffer -- image, row padding and guard rows -- equals the oracle's, and the oracle itself left everything past the frame as it was"""
    guards_kept(want, before, h, what)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d bytes differ, first at row %d byte %d (of %d rows + %d guard rows): got %d want %d" % (
        what, len(bad), bad[0][0], bad[0][1], h, got.shape[0] - h, got[tuple(bad[0])], want[tuple(bad[0])])


def planes_of(pal, w, h, pad, rng=None):
    """plane arrays of a YUV palette with GUARD rows behind each"""
    out = []
    for (nb, rows) in po.YUV_PLANE_DIMS[pal](w, h):
        out.append(np.full((rows + GUARD, nb + pad), FILL, np.uint8) if rng is None else rng.integers(0, 256, (rows + GUARD, nb + pad), dtype=np.uint8))
    return out


def ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


# ---------------------------------------------------------------------------------------------- the cap table against the sources
TERNARIES = [re.compile(r"(\w+)\s*<\s*(\d+)u?\s*\?\s*\1\s*:\s*\2u?\b"), re.compile(r"(\w+)\s*>\s*(\d+)u?\s*\?\s*\2u?\s*:\s*\1\b")]
CLAMP_IF = re.compile(r"if\s*\(\s*(gy|g)\s*>\s*(\d+)\s*\)\s*\1\s*=\s*\2\b")
# a ternary counts on a line that declares a dim3, or where it is the value assigned to gy / g (behind a cast at most): `g = lut16[ig > 65535 ? 65535 : ig]` in yuv.hip
# assigns to a g as well and is no grid
ASSIGNED = re.compile(r"\b(?:gy|g)\s*=\s*(?:\(\s*\w+\s*\)\s*)?\(?\s*$")


def caps_in(line):
    out = [int(m.group(2)) for m in CLAMP_IF.finditer(line)]
    for rx in TERNARIES:
        for m in rx.finditer(line):
            if re.search(r"\bdim3\b", line) or ASSIGNED.search(line[:m.start()]):
                out.append(int(m.group(2)))
    return out


def scan_caps():
    found = collections.Counter()
    for path in sorted(glob.glob(os.path.join(ROOT, "lives_amd", "csrc", "*.hip"))):
        with open(path) as f:
            for line in f:
                for n in caps_in(line):
                    found[(os.path.basename(path), n)] += 1
    return found


def test_the_scan_reads_the_idioms():
    assert caps_in("  const dim3 vgrid(cdiv((unsigned)vw, kBlock), (unsigned)(vh < 1024 ? vh : 1024)), bgrid(cdiv((unsigned)bw, kBlock), (unsigned)(bh < 1024 ? bh : 1024));") == [1024, 1024]
    assert caps_in("  dim3 grid(cdiv((unsigned)(width >> 1), kBlock), (unsigned)(units > 2048 ? 2048 : units), (unsigned)nbatch);") == [2048]
    assert caps_in("  const dim3 tgrid(ntiles < 1024u ? ntiles : 1024u);") == [1024]
    assert caps_in("  unsigned gy = (unsigned)(sh > 2048 ? 2048 : sh);") == [2048] and caps_in("  gy = (unsigned)(dh > 2048 ? 2048 : dh);") == [2048]
    assert caps_in("  if (gy > 4096) gy = 4096;") == [4096] and caps_in("    if (g > 4096) g = 4096;") == [4096]
    assert caps_in("      g = lut16[ig > 65535 ? 65535 : ig < 0 ? 0 : ig] >> 8;") == [] and caps_in("    return c > 255 ? 255 : c < 0 ? 0 : c;") == []
    assert caps_in("    if (g < 1) g = 1;") == []


def test_caps_match_the_sources():
    """every `x < N ? x : N`, `x > N ? N : x` and `if (gy > N) gy = N` on a line that builds a launch grid, per file and N -- and how often: a new launch site or a
    changed cap fails here until CAPS (and with it the heights of this module) follows"""
    want = collections.Counter((f, n) for (f, _), n in CAPS.items())
    found = scan_caps()
    assert found == want, "launch caps in the sources and CAPS differ: only in the sources %s, only in CAPS %s" % (dict(found - want), dict(want - found))
    for (f, kernel), (n, statement) in PER_CU_CAPS.items():
        with open(os.path.join(ROOT, "lives_amd", "csrc", f)) as fh:
            text = fh.read()
        # the file's only product of the CU count is this site's, with this factor
        assert [int(v) for v in re.findall(r"device_cus\(\)\s*\*\s*(\d+)", text)] == [n], "%s: the per-CU caps changed" % f
        assert len(re.findall(statement, text)) == 1, "%s: the launch of %s no longer caps its grid at %d workgroups per CU" % (f, kernel, n)


# ---------------------------------------------------------------------------------------------- swizzle.hip: row_grid
S_ROW = ("swizzle.hip", "row_grid")
SWIZZLE_CASES = [(op, form, h, int(h > 2 * 4096) ^ int(form == "b")) for op in ("swap3", "swap3addpost", "delpost", "swap3postalpha") for form in "vb" for h in heights(S_ROW)]


def run_swizzle(orc, gpu, opname, form, h, use_lut):
    op = po.OPS.index(opname)
    ib, ob, w = po.OP_IBPP[op], po.OP_OBPP[op], W[form]
    rng = seeded("swizzle", opname, form, h)
    lut = rng.integers(0, 256, 256, dtype=np.uint8) if use_lut else None
    src = src_frame(rng, w, h, ib, pitch(w, ib, form))
    before = blank(h, pitch(w, ob, form))
    want = before.copy()
    orc.orc_swizzle(op, 0, P(src), src.strides[0], P(want), want.strides[0], w, h, P(lut))
    wip = None
    if ib == ob:
        wip = src.copy()
        orc.orc_swizzle(op, 0, P(wip), wip.strides[0], P(wip), wip.strides[0], w, h, P(lut))
    if gpu is None:
        return
    d = dev(before)
    gpu.swizzle(op, dev(src), d, w, h, lut=lut)
    same_whole(host(d), want, before, h, "%s %s %d rows" % (opname, form, h))
    if wip is not None:
        d = dev(src)
        gpu.swizzle(op, d, d, w, h, lut=lut)
        same_whole(host(d), wip, src, h, "%s %s %d rows in place" % (opname, form, h))


@G
@pytest.mark.parametrize("case", SWIZZLE_CASES, ids=lambda c: "row_grid-%s-%s-%d" % c[:3])
def test_swizzle(gpu, orc, case):
    """swizzle.hip row_grid: k_swizzle<3|4, 3|4> ("v") and k_swizzle_bytes ("b"), with and without the LUT, out of place and in place"""
    run_swizzle(orc, gpu, *case)


GAMMA_CASES = [(ps, af, form, h) for (ps, af) in ((3, 0), (4, 0), (4, 1)) for form in "vb" for h in heights(S_ROW)]


def run_gamma(orc, gpu, ps, af, form, h):
    w = W[form]
    rng = seeded("gamma", ps, af, form, h)
    lut = rng.integers(0, 256, 256, dtype=np.uint8)
    pix = src_frame(rng, w, h, ps, pitch(w, ps, form))
    want = pix.copy()
    orc.orc_gamma_apply(P(want), want.strides[0], w, h, ps, af, P(lut))
    if gpu is None:
        return
    d = dev(pix)
    gpu.gamma_apply(d, w, h, ps, lut, alpha_first=af)
    same_whole(host(d), want, pix, h, "gamma ps=%d af=%d %s %d rows" % (ps, af, form, h))


@G
@pytest.mark.parametrize("case", GAMMA_CASES, ids=lambda c: "row_grid-ps%d-af%d-%s-%d" % c)
def test_gamma_apply(gpu, orc, case):
    """swizzle.hip row_grid: k_gamma_apply ("v") and k_gamma_apply_bytes ("b"), in place as the entry point is"""
    run_gamma(orc, gpu, *case)


PREMULT_CASES = [(af, un, form, h) for af in (0, 1) for un in (0, 1) for form in "vb" for h in heights(S_ROW)]


def run_premult(orc, gpu, af, un, form, h):
    w = W[form]
    rng = seeded("premult", af, un, form, h)
    pix = frame(rng, w, h, 4, stride=pitch(w, 4, form), extra_rows=GUARD, alpha_mix=True)
    want = pix.copy()
    orc.orc_alpha_premult(P(want), want.strides[0], w, h, af, un)
    if gpu is None:
        return
    d = dev(pix)
    gpu.alpha_premult(d, w, h, alpha_first=af, un=un)
    same_whole(host(d), want, pix, h, "premult af=%d un=%d %s %d rows" % (af, un, form, h))


@G
@pytest.mark.parametrize("case", PREMULT_CASES, ids=lambda c: "row_grid-af%d-un%d-%s-%d" % c)
def test_alpha_premult(gpu, orc, case):
    """swizzle.hip row_grid: k_premult<true> ("v") and k_premult<false> ("b"), in place as the entry point is"""
    run_premult(orc, gpu, *case)


BYTE_LUTS_CASES = [(ps, form, h) for ps in (3, 4) for form in "vb" for h in heights(S_ROW)]


def run_byte_luts(orc, gpu, ps, form, h):
    w = W[form]
    rng = seeded("byte_luts", ps, form, h)
    luts = rng.integers(0, 256, (ps, 256), dtype=np.uint8)
    src = src_frame(rng, w, h, ps, pitch(w, ps, form))
    before = blank(h, src.strides[0])
    want, wip = before.copy(), src.copy()
    orc.orc_byte_luts(P(src), src.strides[0], P(want), want.strides[0], w, h, ps, luts.ctypes.data)
    orc.orc_byte_luts(P(wip), wip.strides[0], P(wip), wip.strides[0], w, h, ps, luts.ctypes.data)
    if gpu is None:
        return
    d = dev(before)
    gpu.byte_luts(dev(src), d, w, h, ps, luts)
    same_whole(host(d), want, before, h, "byte_luts ps=%d %s %d rows" % (ps, form, h))
    d = dev(src)
    gpu.byte_luts(d, d, w, h, ps, luts)
    same_whole(host(d), wip, src, h, "byte_luts ps=%d %s %d rows in place" % (ps, form, h))


@G
@pytest.mark.parametrize("case", BYTE_LUTS_CASES, ids=lambda c: "row_grid-ps%d-%s-%d" % c)
def test_byte_luts(gpu, orc, case):
    """swizzle.hip row_grid: k_byte_luts<3> / <4> at 16 and 13 pixels, out of place and in place"""
    run_byte_luts(orc, gpu, *case)


PREMULT_YUVA_CASES = [(pal, cl, un, form, h) for (pal, cl, form) in ((589, 1, "v"), (589, 0, "v"), (589, 1, "b"), (545, 1, "v"), (545, 0, "b"))
                      for un in (0, 1) for h in heights(S_ROW)]


def run_premult_yuva(orc, gpu, pal, clamped, un, form, h):
    w = W[form]
    rng = seeded("premult_yuva", pal, clamped, un, form, h)
    planes = [src_frame(rng, w, h, 4, pitch(w, 4, form))] if pal == 589 else [src_frame(rng, w, h, 1, pitch(w, 1, form)) for _ in range(4)]
    want = [p.copy() for p in planes]
    pp = (ctypes.c_void_p * 4)(*([x.ctypes.data for x in want] + [None] * (4 - len(want))))
    ss = (ctypes.c_int * 4)(*([x.strides[0] for x in want] + [0] * (4 - len(want))))
    orc.orc_alpha_premult_yuva(pp, ss, w, h, pal, clamped, un)
    if gpu is None:
        return
    ds = [dev(p) for p in planes]
    gpu.alpha_premult_yuva(ds, w, h, pal, clamped, un=un)
    for i in range(len(planes)):
        same_whole(host(ds[i]), want[i], planes[i], h, "premult yuva pal=%d clamped=%d un=%d %s %d rows plane %d" % (pal, clamped, un, form, h, i))


@G
@pytest.mark.parametrize("case", PREMULT_YUVA_CASES, ids=lambda c: "row_grid-%d-cl%d-un%d-%s-%d" % c)
def test_alpha_premult_yuva(gpu, orc, case):
    """swizzle.hip row_grid: k_premult_yuva<1> (clamped YUVA8888, 16 pixels, aligned) and k_premult_yuva<0> (unclamped, 13 pixels, planar), in place"""
    run_premult_yuva(orc, gpu, *case)


SWIZZLE_BATCH_CASES = [("swap3addpost", "v"), ("swap3postalpha", "b")]


def run_swizzle_batch(orc, gpu, opname, form):
    op = po.OPS.index(opname)
    ib, ob, w, n = po.OP_IBPP[op], po.OP_OBPP[op], W[form], 3
    h = heights(S_ROW)[1]
    rng = seeded("swizzle_batch", opname, form)
    srcs = [src_frame(rng, w, h, ib, pitch(w, ib, form)) for _ in range(n)]
    before = blank(h, pitch(w, ob, form))
    wants = []
    for s in srcs:
        wt = before.copy()
        orc.orc_swizzle(op, 0, P(s), s.strides[0], P(wt), wt.strides[0], w, h, None)
        wants.append(wt)
    if gpu is None:
        return
    d_s, d_o = [dev(s) for s in srcs], [dev(before) for _ in range(n)]
    gpu.lib.call("lgpu_swizzle_batch", op, 0, ptrs(d_s), srcs[0].strides[0], ptrs(d_o), before.strides[0], w, h, None, n, None)
    for f in range(n):
        same_whole(host(d_o[f]), wants[f], before, h, "%s batch %s frame %d" % (opname, form, f))


@G
@pytest.mark.parametrize("case", SWIZZLE_BATCH_CASES, ids=lambda c: "row_grid-batch-%s-%s" % c)
def test_swizzle_batch(gpu, orc, case):
    """swizzle.hip row_grid with grid.z: lgpu_swizzle_batch, three frames of 8229 rows, every frame against the oracle"""
    run_swizzle_batch(orc, gpu, *case)


# ---------------------------------------------------------------------------------------------- effects.hip: row_grid2
S_ROW2 = ("effects.hip", "row_grid2")
# (kind, psize, extra): chroma (extra = alpha first), luma (extra = type), multi (extra = type), colorkey
PIXEL2_CASES = [(kind, ps, extra, form, h) for (kind, ps, extra) in (("chroma", 3, 0), ("chroma", 4, 0), ("chroma", 4, 1), ("luma", 3, 1), ("luma", 4, 3), ("multi", 3, 0), ("multi", 3, 5),
                                                                     ("colorkey", 3, 0)) for form in "vb" for h in heights(S_ROW2)]


def run_pixel2(orc, gpu, kind, ps, extra, form, h):
    w = W[form]
    rng = seeded("pixel2", kind, ps, extra, form, h)
    st = pitch(w, ps, form)
    s1 = frame(rng, w, h, ps, stride=st, extra_rows=GUARD, alpha_mix=True)
    s2 = frame(rng, w, h, ps, stride=st, extra_rows=GUARD, alpha_mix=True)
    before = blank(h, st)
    bf = 100

    def oracle(a, out, inplace):
        if kind == "chroma":
            orc.orc_blend_chroma(P(a), st, P(s2), st, P(out), st, w, h, ps, extra, bf)
        elif kind == "luma":
            orc.orc_blend_luma(extra, P(a), st, P(s2), st, P(out), st, w, h, ps, 0, bf, inplace)
        elif kind == "multi":
            orc.orc_blend_multi(extra, P(a), st, P(s2), st, P(out), st, w, h, 0, bf)
        else:
            orc.orc_colorkey(P(a), st, P(s2), st, P(out), st, w, h, 0, 0.35, 0.7, 40, 200, 90, 0)

    def launch(d1, d2, dd):
        if kind == "chroma":
            gpu.blend_chroma(d1, d2, dd, w, h, ps, bf, alpha_first=extra)
        elif kind == "luma":
            gpu.blend_luma(extra, d1, d2, dd, w, h, ps, 0, bf)
        elif kind == "multi":
            gpu.blend_multi(extra, d1, d2, dd, w, h, 0, bf)
        else:
            gpu.colorkey(d1, d2, dd, w, h, 0, 0.35, 0.7, (40, 200, 90))

    want, wip = before.copy(), s1.copy()
    oracle(s1, want, 0)
    oracle(wip, wip, 1)
    if gpu is None:
        return
    d = dev(before)
    launch(dev(s1), dev(s2), d)
    same_whole(host(d), want, before, h, "%s ps=%d %s %s %d rows" % (kind, ps, extra, form, h))
    d = dev(s1)
    launch(d, dev(s2), d)
    same_whole(host(d), wip, s1, h, "%s ps=%d %s %s %d rows in place" % (kind, ps, extra, form, h))


@G
@pytest.mark.parametrize("case", PIXEL2_CASES, ids=lambda c: "row_grid2-%s-ps%d-%d-%s-%d" % c)
def test_blends(gpu, orc, case):
    """effects.hip row_grid2: k_pixel2<3 | 4> with the chroma, luma, multi and colour-key functors, vector ("v") and byte ("b") form, and k_chroma_argb
    (chroma, 4-byte pixels, alpha first); out of place and in place"""
    run_pixel2(orc, gpu, *case)


MIRROR_CASES = [(mode, ps, form, h) for mode in (0, 1, 2) for ps in (3, 4) for form in "vb" for h in heights(S_ROW2)]


def run_mirror(orc, gpu, mode, ps, form, h):
    w = W[form]
    rng = seeded("mirror", mode, ps, form, h)
    st = pitch(w, ps, form)
    s = src_frame(rng, w, h, ps, st)
    before = blank(h, st)
    want, wip = before.copy(), s.copy()
    orc.orc_mirror(mode, P(s), st, P(want), st, w, h, ps)
    orc.orc_mirror(mode, P(wip), st, P(wip), st, w, h, ps)
    if gpu is None:
        return
    d = dev(before)
    gpu.mirror(mode, dev(s), d, w, h, ps)
    same_whole(host(d), want, before, h, "mirror mode=%d ps=%d %s %d rows" % (mode, ps, form, h))
    d = dev(s)
    gpu.mirror(mode, d, d, w, h, ps)
    same_whole(host(d), wip, s, h, "mirror mode=%d ps=%d %s %d rows in place" % (mode, ps, form, h))


@G
@pytest.mark.parametrize("case", MIRROR_CASES, ids=lambda c: "row_grid2-mode%d-ps%d-%s-%d" % c)
def test_mirror(gpu, orc, case):
    """effects.hip row_grid2: k_mirror_v4 (4-byte pixels, "v"), k_mirror<4> ("b") and k_mirror<3>; the vertical modes read row h - 1 - y; out of place and in place"""
    run_mirror(orc, gpu, *case)


LETTERBOX_CASES = [(ps, form, h) for ps in (1, 3, 4) for form in "vb" for h in heights(S_ROW2)]
BLACK = {1: [16, 0, 0, 0], 3: [1, 2, 3, 0], 4: [0, 0, 0, 255]}


def run_letterbox(orc, gpu, ps, form, nh):
    nw = W[form]
    w, h = nw - 5, nh - 35
    rng = seeded("letterbox", ps, form, nh)
    src = src_frame(rng, w, h, ps, pitch(w, ps, form))
    before = blank(nh, pitch(nw, ps, form))
    want = before.copy()
    bp = np.array(BLACK[ps], np.uint8)
    orc.orc_letterbox(P(src), src.strides[0], w, h, P(want), want.strides[0], nw, nh, ps, P(bp))
    bars = src_frame(rng, nw, nh, ps, pitch(nw, ps, form))
    ox, oy = 3, nh - h - 11
    wbars = bars.copy()
    inner = wbars[oy:oy + h, ox * ps:(ox + w) * ps].copy()
    wbars[:nh, :nw * ps] = np.tile(bp[:ps], nw)
    wbars[oy:oy + h, ox * ps:(ox + w) * ps] = inner
    if gpu is None:
        return
    d = dev(before)
    gpu.letterbox(dev(src), d, w, h, nw, nh, ps, BLACK[ps])
    same_whole(host(d), want, before, nh, "letterbox ps=%d %s %d rows" % (ps, form, nh))
    d = dev(bars)
    gpu.lib.call("lgpu_letterbox_bars", d.data_ptr(), d.stride(0), nw, nh, ps, (ctypes.c_uint8 * 4)(*BLACK[ps]), ox, oy, w, h, None)
    same_whole(host(d), wbars, bars, nh, "letterbox bars ps=%d %s %d rows" % (ps, form, nh))


@G
@pytest.mark.parametrize("case", LETTERBOX_CASES, ids=lambda c: "row_grid2-ps%d-%s-%d" % c)
def test_letterbox_and_bars(gpu, orc, case):
    """effects.hip row_grid2: k_letterbox<1 | 3 | 4> against the oracle and k_letterbox_bars<1 | 3 | 4> against a numpy fill (everything but the inner rectangle)"""
    run_letterbox(orc, gpu, *case)


# ---------------------------------------------------------------------------------------------- palette.hip: K4 / K3
S_K4 = ("palette.hip", "k_rgb_to_yuv")
K4_CASES = [(order, ia, w, fmt, h) for fmt in range(6) for (order, ia, w) in ((0, 1, 18), (1, 0, 22), (2, 1, 18)) if not (fmt >= 4 and order == 2)
            for h in heights(S_K4, unit=2 if fmt == 4 else 1)]


def k4_blank(w, h, fmt, oa):
    _, dims = po.k4_out_planes(FILL, w, h, fmt, oa, compact=False)
    return [blank(b, align(a, 16)) for (a, b) in dims], dims


def run_rgb_to_yuv(orc, gpu, order, ia, w, fmt, h, nframes=1):
    rng = seeded("rgb_to_yuv", order, ia, w, fmt, h, nframes)
    ips = 4 if (order == 2 or ia) else 3
    oa = 1 if (fmt <= 1 and order == 0) else 0
    which = (1 if order == 1 else 0) | (2 if (fmt >= 4 and ia) else 0)
    srcs = [src_frame(rng, w, h, ips, align(w * ips)) for _ in range(nframes)]
    before, dims = k4_blank(w, h, fmt, oa)
    wants = []
    for s in srcs:
        wt = [b.copy() for b in before]
        wp, ws = po.planes_args(wt)
        assert orc.orc_rgb_to_yuv(P(s), s.strides[0], w, h, order, ia, ctypes.addressof(wp), ctypes.addressof(ws), fmt, oa, which) == 0
        wants.append(wt)
    for f, wt in enumerate(wants):
        for i, (a, b) in enumerate(dims):
            guards_kept(wt[i], before[i], b, "rgb_to_yuv fmt=%d %dx%d frame %d plane %d" % (fmt, w, h, f, i))
    if gpu is None:
        return
    got = [[dev(b) for b in before] for _ in range(nframes)]
    if nframes == 1:
        gpu.rgb_to_yuv(dev(srcs[0]), got[0], w, h, order, ia, fmt, oa, which)
    else:
        gpu.rgb_to_yuv_batch([dev(s) for s in srcs], got, w, h, order, ia, fmt, oa, which)
    for f in range(nframes):
        for i, (a, b) in enumerate(dims):
            same_whole(host(got[f][i]), wants[f][i], before[i], b, "rgb_to_yuv order=%d alpha=%d fmt=%d %dx%d frame %d plane %d" % (order, ia, fmt, w, h, f, i))


@G
@pytest.mark.parametrize("case", K4_CASES, ids=lambda c: "k_rgb_to_yuv-order%d-alpha%d-w%d-fmt%d-%d" % c)
def test_rgb_to_yuv(gpu, orc, case):
    """palette.hip k_rgb_to_yuv<order, fmt>: widths 18 and 22 (width & 3 != 0), 3- and 4-byte pixels, the six targets; 4:2:0 strides over row pairs"""
    run_rgb_to_yuv(orc, gpu, *case)


@G
@pytest.mark.parametrize("fmt", [2, 4])
def test_rgb_to_yuv_batch(gpu, orc, fmt):
    """palette.hip k_rgb_to_yuv with grid.z: lgpu_rgb_to_yuv_batch, three frames at the taller height (UYVY, and 4:2:0 over row pairs), every frame against the oracle"""
    run_rgb_to_yuv(orc, gpu, 0, 1, 18, fmt, heights(S_K4, unit=2 if fmt == 4 else 1)[1], nframes=3)


S_K3 = ("palette.hip", "k_yuv_to_rgb")
K3_CASES = [(fmt, ia, order, oa, w, h) for (fmt, ia, order, oa, w) in ((0, 0, 0, 0, 22), (0, 1, 1, 1, 18), (0, 1, 2, 1, 21), (1, 0, 0, 1, 18), (1, 1, 1, 1, 22), (1, 1, 0, 0, 21),
                                                                       (2, 0, 0, 0, 18), (2, 0, 2, 1, 22), (3, 0, 1, 0, 22), (3, 0, 0, 1, 18)) for h in heights(S_K3)]


def run_yuv_to_rgb(orc, gpu, fmt, ia, order, oa, w, h):
    rng = seeded("yuv_to_rgb", fmt, ia, order, oa, w, h)
    which = (1 if oa else 0) | (2 if (fmt == 0 and ia) else 0)
    if fmt == 0:
        planes = [src_frame(rng, w, h, 4 if ia else 3, align(w * (4 if ia else 3)))]
    elif fmt == 1:
        planes = [src_frame(rng, w, h, 1, align(w)) for _ in range(4 if ia else 3)]
    else:
        planes = [src_frame(rng, w, h, 2, align(w * 2))]
    ops = 4 if (order == 2 or oa) else 3
    before = blank(h, align(w * ops + 16))
    want = before.copy()
    sp, ss = po.planes_args(planes)
    assert orc.orc_yuv_to_rgb(ctypes.addressof(sp), ctypes.addressof(ss), w, h, fmt, ia, P(want), want.strides[0], order, oa, which) == 0
    guards_kept(want, before, h, "yuv_to_rgb fmt=%d %dx%d" % (fmt, w, h))
    if gpu is None:
        return
    d = dev(before)
    gpu.yuv_to_rgb([dev(a) for a in planes], d, w, h, fmt, ia, order, oa, which)
    same_whole(host(d), want, before, h, "yuv_to_rgb fmt=%d ia=%d order=%d oa=%d %dx%d" % (fmt, ia, order, oa, w, h))


@G
@pytest.mark.parametrize("case", K3_CASES, ids=lambda c: "k_yuv_to_rgb-fmt%d-ia%d-order%d-oa%d-w%d-%d" % c)
def test_yuv_to_rgb(gpu, orc, case):
    """palette.hip k_yuv_to_rgb<fmt, order>: widths 18, 21 and 22 (width & 3 != 0), the four sources, 3- and 4-byte targets"""
    run_yuv_to_rgb(orc, gpu, *case)


S_411 = ("palette.hip", "k_rgb_to_yuv411")
RGB411_CASES = [(order, ia, w, h) for (order, ia, w) in ((0, 0, 22), (1, 1, 20), (2, 1, 23)) for h in heights(S_411)]


def run_rgb_to_yuv411(orc, gpu, order, ia, w, h):
    rng = seeded("rgb411", order, ia, w, h)
    ips = 4 if ia else 3
    src = src_frame(rng, w, h, ips, align(w * ips))
    before = blank(h, (w >> 2) * 6)
    want = before.copy()
    assert orc.orc_rgb_to_yuv411(P(src), src.strides[0], w, h, order, ia, P(want), flag(h)) == 0
    guards_kept(want, before, h, "rgb_to_yuv411 %dx%d" % (w, h))
    if gpu is None:
        return
    d = dev(before)
    gpu.rgb_to_yuv411(dev(src), d, w, h, in_order=order, in_alpha=ia, unclamped=flag(h))
    same_whole(host(d), want, before, h, "rgb_to_yuv411 order=%d alpha=%d %dx%d" % (order, ia, w, h))


@G
@pytest.mark.parametrize("case", RGB411_CASES, ids=lambda c: "k_rgb_to_yuv411-order%d-alpha%d-w%d-%d" % c)
def test_rgb_to_yuv411(gpu, orc, case):
    """palette.hip k_rgb_to_yuv411: compact 4:1:1 rows out of 3- and 4-byte frames whose right edge is cut"""
    run_rgb_to_yuv411(orc, gpu, *case)


def run_repack(orc, gpu, ip, op, w, h, pad, unc, sampling, what):
    rng = seeded("repack", ip, op, w, h, pad, unc, sampling)
    src = planes_of(ip, w, h, pad, rng)
    before = planes_of(op, w, h, pad)
    want = [b.copy() for b in before]
    sp, ss = po.planes_args(src)
    wp, ws = po.planes_args(want)
    assert orc.orc_yuv_repack(ip, op, ctypes.addressof(sp), ctypes.addressof(ss), ctypes.addressof(wp), ctypes.addressof(ws), w, h, unc, sampling) == 0, what
    for i, (nb, rows) in enumerate(po.YUV_PLANE_DIMS[op](w, h)):
        guards_kept(want[i], before[i], rows, "%s %d->%d %dx%d plane %d" % (what, ip, op, w, h, i))
    if gpu is None:
        return
    dst = [dev(b) for b in before]
    gpu.yuv_repack(ip, op, [dev(a) for a in src], dst, w, h, unc, sampling)
    for i, (nb, rows) in enumerate(po.YUV_PLANE_DIMS[op](w, h)):
        same_whole(host(dst[i]), want[i], before[i], rows, "%s %d->%d %dx%d unclamped=%d pad=%d plane %d" % (what, ip, op, w, h, unc, pad, i))


S_411R = ("palette.hip", "k_yuv411_repack")
R411_CASES = [(ip, op, padok, h) for (ip, op, padok) in po.YUV411_REPACK_PAIRS for h in heights(S_411R, even=True)]


def run_r411(orc, gpu, ip, op, padok, h):
    # 4:1:1 pairs: the padding is the source's only (compact destination), so the two sides get their own plane lists
    w, pad, unc = 20, (24 if padok else 0), (ip + op) & 1 ^ flag(h)
    rng = seeded("r411", ip, op, h)
    src = planes_of(ip, w, h, pad, rng)
    before = planes_of(op, w, h, 0)
    want = [b.copy() for b in before]
    sp, ss = po.planes_args(src)
    wp, ws = po.planes_args(want)
    assert orc.orc_yuv_repack(ip, op, ctypes.addressof(sp), ctypes.addressof(ss), ctypes.addressof(wp), ctypes.addressof(ws), w, h, unc, 0) == 0
    if gpu is None:
        return
    dst = [dev(b) for b in before]
    gpu.yuv_repack(ip, op, [dev(a) for a in src], dst, w, h, unc)
    for i, (nb, rows) in enumerate(po.YUV_PLANE_DIMS[op](w, h)):
        same_whole(host(dst[i]), want[i], before[i], rows, "411 repack %d->%d %dx%d unclamped=%d pad=%d plane %d" % (ip, op, w, h, unc, pad, i))


@G
@pytest.mark.parametrize("case", R411_CASES, ids=lambda c: "k_yuv411_repack-%d-%d-pad%d-%d" % c)
def test_yuv411_repack(gpu, orc, case):
    """palette.hip k_yuv411_repack: every 4:1:1 pair at 20 pixels (5 macropixels), even heights for the 4:2:0 sides, padded source rows where the pair takes them"""
    run_r411(orc, gpu, *case)


S_CUP = ("palette.hip", "k_chroma_up_packed")
CUP_CASES = [(ip, op, sampling, h) for (ip, op) in po.CHROMA_UP_PAIRS for sampling in (0, 1) for h in heights(S_CUP, even=True)]


def run_cup(orc, gpu, ip, op, sampling, h):
    run_repack(orc, gpu, ip, op, 18, h, 24, flag(h), sampling, "chroma up")


@G
@pytest.mark.parametrize("case", CUP_CASES, ids=lambda c: "k_chroma_up_packed-%d-%d-sampling%d-%d" % c)
def test_chroma_up_packed(gpu, orc, case):
    """palette.hip k_chroma_up_packed: 4:2:0 / 4:2:2 planar -> packed 4:4:4, both chroma sitings, padded planes, 18 pixels"""
    run_cup(orc, gpu, *case)


S_RPK = ("palette.hip", "k_yuv_repack")
# the pairs that go through the K1 swizzles (588 <-> 589) have no kernel of their own here
RPK_PAIRS = [p for p in po.YUV_REPACK_PAIRS if (p[0], p[1]) not in ((588, 589), (589, 588))]
RPK_CASES = [(ip, op, padok, h) for (ip, op, padok) in RPK_PAIRS for h in heights(S_RPK, unit=2 if op in (512, 513) else 1, even=True)]


def run_rpk(orc, gpu, ip, op, padok, h):
    run_repack(orc, gpu, ip, op, 18, h, 24 if padok else 0, (ip + op) & 1 ^ flag(h), 0, "repack")


@G
@pytest.mark.parametrize("case", RPK_CASES, ids=lambda c: "k_yuv_repack-%d-%d-pad%d-%d" % c)
def test_yuv_repack(gpu, orc, case):
    """palette.hip k_yuv_repack: every pair at 18 pixels (width & 3 != 0, so k_combine_s, k_split_s, k_swab_s, k_pk_to_s, k_888_to_s, k_420_to_422p_s and
    k_420_to_packed_s all decline), padded planes where the pair takes them; 4:2:0 targets stride over row pairs and 2x2 blocks"""
    run_rpk(orc, gpu, *case)


# ---------------------------------------------------------------------------------------------- yuv.hip
S_K2 = ("yuv.hip", "k_yuv420p_to_rgb")
# 4:2:0: units = height / 2 + 1 (row 0, the row pairs, the trailing row): an even height of 2 C puts exactly the trailing row into the second trip, 2 C + 2 also sends
# blockIdx.y = 1 -- whose first unit came from the prefetched samples -- on a second trip; 2 C + 1 is an odd height
K2_H = {0: [2 * CAPS[S_K2], 2 * (2 * CAPS[S_K2] + 37) - 2, 2 * CAPS[S_K2] + 2, 2 * CAPS[S_K2] + 1], 1: heights(S_K2)}
K2_CASES = [(opsize, q, lut, order, is422, fix, h) for (opsize, q, lut, order) in ((3, 2, 0, 0), (3, 3, 1, 1), (4, 1, 1, 0), (4, 1, 0, 2)) for is422 in (0, 1)
            for fix in ((0, 1) if not is422 else (0,)) for h in K2_H[is422]]


def l2s_lut(orc):
    lut = np.zeros(256, np.uint8)
    assert orc.orc_gamma_lut8(1.0, po.GAMMA_LINEAR, po.GAMMA_SRGB, 1.4, P(lut)) == 1
    return lut


def k2_planes(rng, w, h, is422):
    ch = h if is422 else h // 2
    return (rng.integers(0, 256, (h, 32), dtype=np.uint8), rng.integers(0, 256, (ch, 16), dtype=np.uint8), rng.integers(0, 256, (ch, 16), dtype=np.uint8))


def run_yuv420p(orc, gpu, opsize, q, use_lut, order, is422, fix, h):
    w = 18
    rng = seeded("k2", opsize, q, use_lut, order, is422, fix, h)
    lut = l2s_lut(orc) if use_lut else None
    Y, U, V = k2_planes(rng, w, h, is422)
    before = blank(h, align(w * opsize + 16))
    want = before.copy()
    strides = (ctypes.c_int * 3)(32, 16, 16)
    which = int(rng.integers(0, 4))
    orc.orc_yuv420p_to_rgb(P(Y), P(U), P(V), strides, U.size, V.size, P(want), want.strides[0], w, h, opsize, order, is422, which, q, P(lut), fix)
    if gpu is None:
        return
    d = dev(before)
    gpu.yuv420p_to_rgb(dev(Y), dev(U), dev(V), d, w, h, opsize=opsize, out_order=order, is_422=is422, which_tables=which, pb_quality=q, lut=lut,
                       flags=gpu.lib.YUV_FIX_EDGES if fix else 0)
    same_whole(host(d), want, before, h, "yuv42%dp opsize=%d quality=%d lut=%d order=%d fix=%d %d rows" % (2 if is422 else 0, opsize, q, use_lut, order, fix, h))


@G
@pytest.mark.parametrize("case", K2_CASES, ids=lambda c: "k_yuv420p_to_rgb-ops%d-q%d-lut%d-order%d-422_%d-fix%d-%d" % c)
def test_yuv420p_to_rgb(gpu, orc, case):
    """yuv.hip k_yuv420p_to_rgb (first unit from prefetched samples, then unit += gridDim.y; row 0 and the trailing row) and k_yuv422p_to_rgb: opsize 3, and LOW
    quality with opsize 4 -- the shapes the paired-table form declines; even and odd heights for 4:2:0"""
    run_yuv420p(orc, gpu, *case)


K2_LUT16_CASES = [(is422, order, ops, h) for is422 in (0, 1) for (order, ops) in ((0, 4), (1, 3)) for h in K2_H[is422][:2]]


def run_yuv420p_lut16(orc, gpu, is422, order, ops, h):
    w = 18
    rng = seeded("k2lut16", is422, order, ops, h)
    lut16 = np.zeros(65536, np.uint16)
    assert orc.orc_gamma_lut16(1.0, po.GAMMA_LINEAR, po.GAMMA_SRGB, 1.4, P(lut16)) == 1
    Y, U, V = k2_planes(rng, w, h, is422)
    before = blank(h, align(w * ops + 16))
    want = before.copy()
    st = (ctypes.c_int * 3)(32, 16, 16)
    assert orc.orc_yuv420p_to_rgb_lut16(P(Y), P(U), P(V), st, U.size, V.size, P(want), want.strides[0], w, h, ops, order, is422, 1, 2, P(lut16), 1) == 0
    if gpu is None:
        return
    import torch
    d = dev(before)
    gpu.yuv420p_to_rgb_lut16(dev(Y), dev(U), dev(V), d, w, h, torch.from_numpy(lut16.view(np.int16)).cuda(), opsize=ops, out_order=order, is_422=is422, which_tables=1, flags=1)
    same_whole(host(d), want, before, h, "yuv42%dp lut16 order=%d opsize=%d %d rows" % (2 if is422 else 0, order, ops, h))


@G
@pytest.mark.parametrize("case", K2_LUT16_CASES, ids=lambda c: "k_yuv420p_to_rgb-lut16-422_%d-order%d-ops%d-%d" % c)
def test_yuv420p_to_rgb_lut16(gpu, orc, case):
    """yuv.hip k_yuv420p_to_rgb / k_yuv422p_to_rgb through lgpu_yuv420p_to_rgb_lut16 (the 16-bit LUT inline)"""
    run_yuv420p_lut16(orc, gpu, *case)


# ---------------------------------------------------------------------------------------------- resize.hip
S_RH, S_RV, S_G5 = ("resize.hip", "k_hpass_generic/resize"), ("resize.hip", "k_vpass_generic/resize"), ("resize.hip", "k_hpass_generic+k_vpass_generic/gauss5")
assert CAPS[S_RH] == CAPS[S_RV]
# (psize, misaligned pitch): 4-byte pixels reach the generic passes on a pitch that is 1 byte off alignment
GENERIC_PS = [(1, 0), (3, 0), (4, 1)]
RESIZE_CASES = [(ps, off, tall_src, h) for (ps, off) in GENERIC_PS for tall_src in (1, 0) for h in heights(S_RH)]


def run_resize(orc, gpu, ps, off, tall_src, H):
    # a tall source shrinks by 1.37 (h pass over H rows; the v pass still exceeds the cap at the taller height), a tall destination enlarges by 1.37 (v pass over H rows)
    other = int(H / 1.37)
    sw, sh, dw, dh = (22, H, 15, other) if tall_src else (15, other, 22, H)
    rng = seeded("resize", ps, off, tall_src, H)
    src = src_frame(rng, sw, sh, ps, align(sw * ps) + off)
    before = blank(dh, align(dw * ps + 16) + off)
    want = before.copy()
    assert orc.orc_resize(P(src), src.strides[0], sw, sh, P(want), want.strides[0], dw, dh, ps, 3) == 0
    if gpu is None:
        return
    d = dev(before)
    gpu.resize(dev(src), d, sw, sh, dw, dh, psize=ps, interp=3)
    same_whole(host(d), want, before, dh, "resize ps=%d %dx%d -> %dx%d" % (ps, sw, sh, dw, dh))


@G
@pytest.mark.parametrize("case", RESIZE_CASES, ids=lambda c: "k_hpass_generic-k_vpass_generic-ps%d-off%d-tallsrc%d-%d" % c)
def test_resize(gpu, orc, case):
    """resize.hip k_hpass_generic (tall source) and k_vpass_generic (tall destination) from lgpu_resize: psize 1 and 3, psize 4 on a misaligned pitch; x 1 / 1.37 and x 1.37"""
    run_resize(orc, gpu, *case)


GAUSS5_CASES = [(ps, off, h) for (ps, off) in GENERIC_PS for h in heights(S_G5)]


def run_gauss5(orc, gpu, ps, off, h):
    w = 22
    rng = seeded("gauss5", ps, off, h)
    src = src_frame(rng, w, h, ps, align(w * ps) + off)
    before = blank(h, align(w * ps + 16) + off)
    want = before.copy()
    orc.orc_gauss5(P(src), src.strides[0], P(want), want.strides[0], w, h, ps)
    if gpu is None:
        return
    d = dev(before)
    gpu.gauss5(dev(src), d, w, h, psize=ps)
    same_whole(host(d), want, before, h, "gauss5 ps=%d %dx%d" % (ps, w, h))


@G
@pytest.mark.parametrize("case", GAUSS5_CASES, ids=lambda c: "k_hpass_generic-k_vpass_generic-gauss5-ps%d-off%d-%d" % c)
def test_gauss5(gpu, orc, case):
    """resize.hip k_hpass_generic + k_vpass_generic from lgpu_gauss5: psize 1 and 3 at 22 pixels (width & 3 != 0), psize 4 on a misaligned pitch"""
    run_gauss5(orc, gpu, *case)


# ---------------------------------------------------------------------------------------------- effects.hip: 2048
S_COMP = ("effects.hip", "k_composite")
COMPOSITE_CASES = [(ps, is_bgr, revz, h) for (ps, is_bgr, revz) in ((3, 0, 0), (3, 1, 1), (4, 1, 0), (4, 0, 1)) for h in heights(S_COMP)]


def run_composite(orc, gpu, ps, is_bgr, revz, oh):
    ow, c = 20, CAPS[S_COMP]
    rng = seeded("composite", ps, is_bgr, revz, oh)
    # four layers: across the top edge, across the bottom edge, one inside the rows of the later trips (it starts beyond row C where the frame has such rows, and
    # spans row C at C + 1 rows), and one that covers the frame and crosses both edges
    geo = [(12, 60, -3, -25, 0.7312), (15, 90, 9, oh - 40, 1.0), (8, 300, 5, min(c + 5, oh - 20), 0.5), (25, oh + 10, -2, -5, 0.25)]
    layers = [(src_frame(rng, w, h, ps, align(w * ps)), w, h, ox, oy, al) for (w, h, ox, oy, al) in geo]
    bg = [int(v) for v in rng.integers(0, 256, 3)]
    L = (po.CompLayer * len(layers))()
    for z, (a, w, h, ox, oy, al) in enumerate(layers):
        L[z].src, L[z].irow = a.ctypes.data, a.strides[0]
        L[z].width, L[z].height, L[z].offs_x, L[z].offs_y, L[z].alpha = w, h, ox, oy, al
    before = blank(oh, align(ow * ps + 16))
    want = before.copy()
    orc.orc_composite(P(want), want.strides[0], ow, oh, ps, is_bgr, (ctypes.c_int * 3)(*bg), L, len(layers), revz)
    if gpu is None:
        return
    d = dev(before)
    gpu.composite(d, ow, oh, ps, [(dev(a), w, h, ox, oy, al) for (a, w, h, ox, oy, al) in layers], bgcol=bg, is_bgr=is_bgr, revz=revz)
    same_whole(host(d), want, before, oh, "composite ps=%d bgr=%d revz=%d %d rows" % (ps, is_bgr, revz, oh))


@G
@pytest.mark.parametrize("case", COMPOSITE_CASES, ids=lambda c: "k_composite-ps%d-bgr%d-revz%d-%d" % c)
def test_composite(gpu, orc, case):
    """effects.hip k_composite<3 | 4>: four layers whose offsets cross the top and the bottom of the frame, one of them starting beyond row 2048 (at 2049 rows: across it)"""
    run_composite(orc, gpu, *case)


S_SLIDE, S_SPLIT, S_DISS = ("effects.hip", "k_slide_over"), ("effects.hip", "k_triple_split"), ("effects.hip", "k_dissolve")
TRANSITION_CASES = [(kind, ps, amt, h) for kind in (0, 1, 2) for (ps, amt) in ((3, 0.25), (4, 0.73)) for h in heights(S_SLIDE)]


def run_transition(orc, gpu, kind, ps, amt, h):
    w = 20
    rng = seeded("transition", kind, ps, amt, h)
    st = align(w * ps + 16)
    s1, s2 = src_frame(rng, w, h, ps, st), src_frame(rng, w, h, ps, st)
    before = blank(h, st)
    want = before.copy()
    orc.orc_transition(kind, P(s1), st, P(s2), st, P(want), st, w, h, ps, amt)
    wip = None
    if kind < 2:
        wip = s1.copy()
        orc.orc_transition(kind, P(wip), st, P(s2), st, P(wip), st, w, h, ps, amt)
    if gpu is None:
        return
    d = dev(before)
    gpu.transition(kind, dev(s1), dev(s2), d, w, h, ps, amt)
    same_whole(host(d), want, before, h, "transition %d ps=%d amount=%s %d rows" % (kind, ps, amt, h))
    if wip is not None:
        d = dev(s1)
        gpu.transition(kind, d, dev(s2), d, w, h, ps, amt)
        same_whole(host(d), wip, s1, h, "transition %d ps=%d amount=%s %d rows in place" % (kind, ps, amt, h))


@G
@pytest.mark.parametrize("case", TRANSITION_CASES, ids=lambda c: "k_transition-kind%d-ps%d-%s-%d" % c)
def test_transition(gpu, orc, case):
    """effects.hip k_transition (iris rectangle, iris circle, four-way split): a linear walk, at the heights of its neighbours; in place where the reference allows it"""
    run_transition(orc, gpu, *case)


SLIDE_CASES = [(ps, dirn, tv, mvl, mvu, h) for (ps, dirn, tv, mvl, mvu) in ((3, 1, 60, 1, 0), (4, 2, 128, 0, 1), (3, 3, 200, 1, 1), (4, 4, 77, 1, 0), (4, 3, 254, 0, 0), (3, 4, 1, 0, 1))
               for h in heights(S_SLIDE)]


def run_slide_over(orc, gpu, ps, dirn, tv, mvl, mvu, h):
    w = 20
    rng = seeded("slide", ps, dirn, tv, mvl, mvu, h)
    st = align(w * ps + 16)
    s1, s2 = src_frame(rng, w, h, ps, st), src_frame(rng, w, h, ps, st)
    before = blank(h, st)
    want = before.copy()
    orc.orc_slide_over(P(s1), st, P(s2), st, P(want), st, w, h, ps, tv, dirn, mvl, mvu)
    if gpu is None:
        return
    d = dev(before)
    gpu.slide_over(dev(s1), dev(s2), d, w, h, ps, tv, dirn, mvl, mvu)
    same_whole(host(d), want, before, h, "slide over ps=%d dir=%d amount=%d lower=%d upper=%d %d rows" % (ps, dirn, tv, mvl, mvu, h))


@G
@pytest.mark.parametrize("case", SLIDE_CASES, ids=lambda c: "k_slide_over-ps%d-dir%d-amount%d-lower%d-upper%d-%d" % c)
def test_slide_over(gpu, orc, case):
    """effects.hip k_slide_over<3 | 4>: the four directions (the vertical ones shift rows by a bound that depends on the height); the entry point refuses in-place calls"""
    run_slide_over(orc, gpu, *case)


SPLIT_CASES = [(is_bgr,) + prm + (h,) for (is_bgr, prm) in ((0, (0.666667, 1, 0.333333, 0, 0.)), (1, (0.25, 0, 0.75, 0, 0.04)), (0, (0.4, 1, 0.0, 1, 0.07)), (1, (0.8, 0, 0.3, 1, 0.2)))
               for h in heights(S_SPLIT)]


def run_triple_split(orc, gpu, is_bgr, start, sym, end, vert, bw, h):
    w = 20
    rng = seeded("split", is_bgr, start, sym, end, vert, bw, h)
    bc = np.array([13, 250, 77], np.int32)
    st = align(w * 3 + 16)
    s1, s2 = src_frame(rng, w, h, 3, st), src_frame(rng, w, h, 3, st)
    before = blank(h, st)
    want, wip = before.copy(), s1.copy()
    orc.orc_triple_split(P(s1), st, P(s2), st, P(want), st, w, h, is_bgr, start, sym, end, vert, bw, bc.ctypes.data)
    orc.orc_triple_split(P(wip), st, P(s2), st, P(wip), st, w, h, is_bgr, start, sym, end, vert, bw, bc.ctypes.data)
    if gpu is None:
        return
    d = dev(before)
    gpu.triple_split(dev(s1), dev(s2), d, w, h, is_bgr, start, sym, end, vert, bw, bc)
    same_whole(host(d), want, before, h, "triple split %r %d rows" % ((start, sym, end, vert, bw), h))
    d = dev(s1)
    gpu.triple_split(d, dev(s2), d, w, h, is_bgr, start, sym, end, vert, bw, bc)
    same_whole(host(d), wip, s1, h, "triple split %r %d rows in place" % ((start, sym, end, vert, bw), h))


@G
@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: "k_triple_split-bgr%d-%s-%d-%s-rows%d-%s-%d" % c)
def test_triple_split(gpu, orc, case):
    """effects.hip k_triple_split: column and row splits (the row borders are fractions of the height), out of place and in place"""
    run_triple_split(orc, gpu, *case)


DISSOLVE_CASES = [(ps, amt, h) for (ps, amt) in ((3, 0.37), (4, 0.5), (4, 0.999)) for h in heights(S_DISS)]


def run_dissolve(orc, gpu, ps, amt, h):
    w = 20
    rng = seeded("dissolve", ps, amt, h)
    seed = 0xC0FFEE + h
    mask = np.zeros(w * h, np.float32)
    orc.orc_dissolve_mask(seed, w, h, mask.ctypes.data)
    st = align(w * ps + 16)
    s1, s2 = src_frame(rng, w, h, ps, st), src_frame(rng, w, h, ps, st)
    before = blank(h, st)
    want, wip = before.copy(), s1.copy()
    orc.orc_dissolve(P(s1), st, P(s2), st, P(want), st, w, h, ps, mask.ctypes.data, amt)
    orc.orc_dissolve(P(wip), st, P(s2), st, P(wip), st, w, h, ps, mask.ctypes.data, amt)
    if gpu is None:
        return
    import torch
    gm = gpu.dissolve_mask(seed, w, h)
    assert (gm == mask).all()
    dm = torch.from_numpy(gm).cuda()
    d = dev(before)
    gpu.dissolve(dev(s1), dev(s2), d, w, h, ps, dm, amt)
    same_whole(host(d), want, before, h, "dissolve ps=%d amount=%s %d rows" % (ps, amt, h))
    d = dev(s1)
    gpu.dissolve(d, dev(s2), d, w, h, ps, dm, amt)
    same_whole(host(d), wip, s1, h, "dissolve ps=%d amount=%s %d rows in place" % (ps, amt, h))


@G
@pytest.mark.parametrize("case", DISSOLVE_CASES, ids=lambda c: "k_dissolve-ps%d-%s-%d" % c)
def test_dissolve(gpu, orc, case):
    """effects.hip k_dissolve<3 | 4>: the mask is indexed by row * width + column; out of place and in place"""
    run_dissolve(orc, gpu, *case)


# ---------------------------------------------------------------------------------------------- stencil.hip
S_DEINT = ("stencil.hip", "k_deinterlace")
# the cap counts row pairs and npairs = (height - 2) >> 1
DEINT_H = [h + 2 for h in heights(S_DEINT, unit=2)]
DEINT_CASES = [(pal, w, inplace, h) for (pal, w) in ((1, 21), (2, 20), (588, 21), (3, 21), (4, 20), (589, 21), (5, 21), (564, 21), (565, 20)) for inplace in ((1,) if pal == 5 else (0, 1))
               for h in DEINT_H]


def run_deinterlace(orc, gpu, pal, w, inplace, h):
    ps = 3 if pal in (1, 2, 588) else 4
    rng = seeded("deinterlace", pal, w, inplace, h)
    s1 = src_frame(rng, w, h, ps, align(w * ps))
    # smooth vertical structure with comb rows so that both branches of the decision occur
    s1[1:h:2] = (s1[1:h:2] >> 2) + 160
    s1[0:h:2] = (s1[0:h:2] >> 2) + (rng.integers(0, 2, (s1[0:h:2].shape[0], 1), dtype=np.uint8) * 120)
    before = s1 if inplace else blank(h, s1.strides[0])
    want = before.copy()
    src = want if inplace else s1
    assert orc.orc_deinterlace(P(src), src.strides[0], P(want), want.strides[0], w, h, pal) == 0
    if gpu is None:
        return
    if inplace:
        d = dev(s1)
        gpu.deinterlace(d, d, w, h, pal)
    else:
        d = dev(before)
        gpu.deinterlace(dev(s1), d, w, h, pal)
    same_whole(host(d), want, before, h, "deinterlace pal=%d %dx%d inplace=%d" % (pal, w, h, inplace))


@G
@pytest.mark.parametrize("case", DEINT_CASES, ids=lambda c: "k_deinterlace-pal%d-w%d-inplace%d-%d" % c)
def test_deinterlace(gpu, orc, case):
    """stencil.hip k_deinterlace: 2049 and 4133 row pairs; whole triples (21 pixels: the dword walk for 4-byte pixels) and a partial last triple (20 pixels), out of
    place and in place (from the per-stream snapshot)"""
    run_deinterlace(orc, gpu, *case)


S_EDGE, S_EMAP = ("stencil.hip", "k_edge_paint"), ("stencil.hip", "k_edge_map")
EDGE_TILE = (64, 16)            # kStW x kStH in stencil.hip: the output tile of a k_edge_map<PS> workgroup
# 68 x 8193: 2 x 513 = 1026 tiles (the second tile column is partial), the smallest frame above 1024 tiles that has more than one tile column
EDGE_MANY = (EDGE_TILE[0] + 4, EDGE_TILE[1] * (CAPS[S_EMAP] // 2) + 1)
EDGE_CASES = [(pal, mode, 20, h) for (pal, mode) in ((1, 0), (2, 2), (3, 1), (4, 2), (5, 0)) for h in heights(S_EDGE)] + [(2, 0) + EDGE_MANY, (3, 2) + EDGE_MANY]


def edge_source(rng, w, h, ps):
    s = src_frame(rng, w, h, ps, align(w * ps + 16))
    yy, xx = np.mgrid[0:h, 0:w]                      # smooth structure under the noise so that the histogram is not flat
    for c in range(ps):
        s[:h, c:w * ps:ps] = ((s[:h, c:w * ps:ps] >> 3) + (96 * ((xx // 9 + yy // 7 + c) % 2)).astype(np.uint8) + 40).astype(np.uint8)
    return s


def run_edge(orc, gpu, tune, pal, mode, w, h, quads=0):
    ps = 3 if pal <= 2 else 4
    rng = seeded("edge", pal, mode, w, h)
    tw, th = EDGE_TILE4 if quads else EDGE_TILE
    assert -(-w // tw) * -(-h // th) > CAPS[S_EMAP] or (h > CAPS[S_EDGE] and not quads)
    s = edge_source(rng, w, h, ps)
    d0 = rng.integers(0, 256, s.shape, dtype=np.uint8)
    want, wip = d0.copy(), s.copy()
    m16 = np.zeros(w * h, np.int16)
    orc.orc_edge(P(s), s.strides[0], P(want), want.strides[0], w, h, pal, mode, P(m16), 0)
    orc.orc_edge(P(wip), wip.strides[0], P(wip), wip.strides[0], w, h, pal, mode, P(m16), 1)
    if gpu is None:
        return
    tune("EDGE_NO_S", 0 if quads else 1)
    if quads:
        import torch
        lanes = torch.cuda.get_device_properties(0).multi_processor_count * PER_CU_CAPS[("stencil.hip", "k_edge_paint4")][0] * 256
        assert (w >> 2) * h > lanes, "%d quads fit the %d lanes of k_edge_paint4's capped grid on this device: the frame no longer reaches its stride" % ((w >> 2) * h, lanes)
    d = dev(d0)
    gpu.edge(dev(s), d, w, h, pal, mode)
    same_whole(host(d), want, d0, h, "edge pal=%d mode=%d %dx%d" % (pal, mode, w, h))
    d = dev(s)
    gpu.edge(d, d, w, h, pal, mode)
    same_whole(host(d), wip, s, h, "edge pal=%d mode=%d %dx%d in place" % (pal, mode, w, h))


@G
@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: "k_edge_map-k_edge_paint-pal%d-mode%d-%dx%d" % c)
def test_edge(gpu, orc, tune, case):
    """stencil.hip k_edge_paint<3 | 4> (1024 rows) and k_edge_map<3 | 4> (1024 workgroups, one histogram slice each: 68 x 8193 has 1026 tiles) with EDGE_NO_S set;
    out of place and in place"""
    run_edge(orc, gpu, tune, *case)


EDGE_TILE4 = (128, 32)          # kEmW x the default tile height of k_edge_map4
assert CAPS[("stencil.hip", "k_edge_map4")] == CAPS[S_EMAP]
# 132 x 16385: 2 x 513 tiles, and 33 x 16385 quads for k_edge_paint4 -- more than 8 x 256 lanes on each of 256 CUs
EDGE4_MANY = (EDGE_TILE4[0] + 4, EDGE_TILE4[1] * (CAPS[S_EMAP] // 2) + 1)
EDGE4_CASES = [(3, 2) + EDGE4_MANY, (5, 0) + EDGE4_MANY]


@G
@pytest.mark.parametrize("case", EDGE4_CASES, ids=lambda c: "k_edge_map4-k_edge_paint4-pal%d-mode%d-%dx%d" % c)
def test_edge_by_quads(gpu, orc, tune, case):
    """stencil.hip k_edge_map4 (1024 workgroups: 1026 tiles of 128 x 32) and k_edge_paint4 (8 workgroups per CU: 540,705 quads), the form lgpu_edge takes for 4-byte
    pixels on 16-byte aligned rows; out of place and in place, guard rows and padding compared"""
    run_edge(orc, gpu, tune, *case, quads=1)


S_BZ = ("stencil.hip", "k_bz_blur+k_bz_zoom")
assert CAPS[S_BZ] == CAPS[("stencil.hip", "k_bz_update+k_bz_color")]
# k_bz_blur walks rows 1 .. height - 2, so C + 2 rows fit its first trip: C + 4 gives it two rows of a second trip
BZ_CASES = [(pal, mode, pattern, h) for (pal, mode, pattern) in ((3, 0, 0), (4, 0, 3), (3, 1, 1), (4, 2, 0), (4, 3, 2)) for h in heights(S_BZ, even=True) + [CAPS[S_BZ] + 4]]


def bz_frames(rng, w, h, n, compact):
    """bright blocks moving over a dim noisy background at several depths of the frame, so that the background subtraction fires above and below row 1024"""
    out = []
    for f in range(n):
        a = src_frame(rng, w, h, 4, w * 4 if compact else align(w * 4 + 16))
        a[:h, :w * 4] = (a[:h, :w * 4] >> 4) + 40
        for y0 in range(2 + 5 * f, h - 8, 331):
            x0 = (8 + 5 * f + y0) % (w - 20)
            a[y0:y0 + 6, x0 * 4:(x0 + 16) * 4] = 250
        out.append(a)
    return out


def run_blurzoom(orc, gpu, pal, mode, pattern, h):
    w = 70
    rng = seeded("blurzoom", pal, mode, pattern, h)
    seq = bz_frames(rng, w, h, 6 if mode == 2 else 4, compact=mode in (1, 2))       # strobe2 leaves k_bz_update out of frames 1 .. 3 and runs it again on frame 4
    z = orc.orc_blurzoom_new(w, h, pal)
    wants = []
    for a in seq:
        want = np.full_like(a, FILL)
        assert orc.orc_blurzoom_process(z, P(a), a.strides[0], P(want), want.strides[0], mode, pattern) == 0
        wants.append(want)
    orc.orc_blurzoom_free(z)
    if gpu is None:
        return
    g = gpu.Blurzoom(w, h, pal)
    try:
        for f, a in enumerate(seq):
            before = np.full_like(a, FILL)
            d = dev(before)
            g.process(dev(a), d, mode, pattern)
            same_whole(host(d), wants[f], before, h, "blurzoom pal=%d mode=%d pattern=%d %dx%d frame %d" % (pal, mode, pattern, w, h, f))
    finally:
        g.close()


@G
@pytest.mark.parametrize("case", BZ_CASES, ids=lambda c: "k_bz-pal%d-mode%d-pattern%d-%d" % c)
def test_blurzoom(gpu, orc, case):
    """stencil.hip k_bz_update, k_bz_blur (starts at blockIdx.y + 1), k_bz_zoom, k_bz_color: four frames of one instance in the normal, strobe and trigger modes,
    six in strobe2 (the mode that skips k_bz_update while its snapshot is fresh)"""
    run_blurzoom(orc, gpu, *case)


S_RGBD = ("stencil.hip", "k_rgbdelay+k_rgbdelay4")
assert CAPS[S_RGBD] == CAPS[("stencil.hip", "k_rgbd_snapshot")]
RGBD_CASES = [(pal, w, inplace, h) for (pal, w, inplace) in ((1, 22, 0), (2, 24, 1), (588, 24, 0), (588, 22, 1)) for h in heights(S_RGBD)]


def run_rgbdelay(orc, gpu, pal, w, inplace, h):
    from tests import golden_util as gu
    rng = seeded("rgbdelay", pal, w, inplace, h)
    # the ring grows to three frames, is re-weighted, then shrinks to two: six frames, a parameter change after every second one
    plans = [({0: (1, 0, 0, 1.0), 1: (0, 1, 0, 0.8), 2: (0, 0, 1, 1.0)}, 4), ({0: (1, 1, 1, 0.5), 2: (1, 0, 1, 0.7)}, 4), ({0: (0, 1, 1, 0.9), 1: (1, 0, 0, 1.0)}, 3)]
    s = orc.orc_rgbdelay_new()
    steps = []
    for groups, maxcache in plans:
        on, st = gu.rgbdelay_params(groups)
        for _ in range(2):
            src = src_frame(rng, w, h, 3, align(w * 3 + 16))
            before = src if inplace else np.full_like(src, FILL)
            want = before.copy()
            a = want if inplace else src
            assert orc.orc_rgbdelay_process(s, P(a), a.strides[0], P(want), want.strides[0], w, h, pal, 1, maxcache, on.ctypes.data, st.ctypes.data) == 0
            steps.append((src, before, want, maxcache, on, st))
    for f, (src, before, want, maxcache, on, st) in enumerate(steps):
        guards_kept(want, before, h, "rgbdelay pal=%d %dx%d frame %d" % (pal, w, h, f))
    orc.orc_rgbdelay_free(s)
    if gpu is None:
        return
    rd = gpu.RgbDelay()
    try:
        for f, (src, before, want, maxcache, on, st) in enumerate(steps):
            ds = dev(src)
            d = ds if inplace else dev(before)
            rd.process(ds, d, w, h, pal, maxcache, on, st, yuv_clamped=True)
            same_whole(host(d), want, before, h, "rgbdelay pal=%d %dx%d inplace=%d frame %d" % (pal, w, h, inplace, f))
    finally:
        rd.close()


@G
@pytest.mark.parametrize("case", RGBD_CASES, ids=lambda c: "k_rgbdelay-k_rgbd_snapshot-pal%d-w%d-inplace%d-%d" % c)
def test_rgbdelay(gpu, orc, case):
    """stencil.hip k_rgbd_snapshot, k_rgbdelay (22 pixels) and k_rgbdelay4 (24 pixels: 3 * width % 4 == 0): six frames through one ring whose parameters change
    after every second frame"""
    run_rgbdelay(orc, gpu, *case)


# ---------------------------------------------------------------------------------------------- runtime.hip
S_FILL = ("runtime.hip", "k_fill_pattern")
FILL_CASES = [(plen, rows) for plen in (1, 3, 4, 8) for rows in heights(S_FILL)]
assert heights(S_FILL) == [513, 1061]


@G
@pytest.mark.parametrize("plen,rows", FILL_CASES, ids=lambda v: str(v))
def test_fill_pattern(gpu, plen, rows):
    """runtime.hip k_fill_pattern through lgpu_fill_pattern, and lgpu_fill (a memset) and lgpu_letterbox_bars at the same row counts, against numpy fills.  k_set4 and
    k_set64 are single-workgroup launches of at most 64 values and have no walk to stride"""
    rng = seeded("fill", plen, rows)
    n, stride = 7, 7 * plen + 9
    before = rng.integers(0, 256, (rows + GUARD, stride), dtype=np.uint8)
    pat = rng.integers(0, 256, plen, dtype=np.uint8)
    want = before.copy()
    want[:rows, :n * plen] = np.tile(pat, n)
    d = dev(before)
    gpu.lib.call("lgpu_fill_pattern", d.data_ptr(), stride, pat.ctypes.data, plen, n, rows, None)
    same_whole(host(d), want, before, rows, "fill_pattern plen=%d %d rows" % (plen, rows))
    d = dev(before)
    gpu.lib.call("lgpu_fill", d.data_ptr(), 0x3C, rows * stride, None)
    want = before.copy()
    want[:rows] = 0x3C
    same_whole(host(d), want, before, rows, "fill %d rows" % rows)
    if plen in (1, 3, 4):
        canvas = rng.integers(0, 256, (rows + GUARD, 13 * plen + 3 + plen), dtype=np.uint8)
        canvas = canvas[:, :(canvas.shape[1] // 4) * 4] if plen == 4 else canvas
        canvas = np.ascontiguousarray(canvas)
        want = canvas.copy()
        want[:rows, :13 * plen] = np.tile(pat, 13)
        want[5:rows - 9, 2 * plen:12 * plen] = canvas[5:rows - 9, 2 * plen:12 * plen]
        d = dev(canvas)
        b = (ctypes.c_uint8 * 4)(*(list(pat) + [0] * (4 - plen)))
        gpu.lib.call("lgpu_letterbox_bars", d.data_ptr(), d.stride(0), 13, rows, plen, b, 2, 5, 10, rows - 14, None)
        same_whole(host(d), want, canvas, rows, "letterbox bars ps=%d %d rows" % (plen, rows))


# ---------------------------------------------------------------------------------------------- the two walks that are not row walks
def run_yuv411_to_rgb_4k(orc, gpu, order, oa, uncl):
    wm, h = 3840 // 4, 2160
    ps = 4 if (order == 2 or oa) else 3
    rng = seeded("yuv411_4k", order, oa, uncl)
    src = rng.integers(0, 256, (h, wm * 6), dtype=np.uint8)
    before = blank(h, wm * 4 * ps + 32)
    want = before.copy()
    assert orc.orc_yuv411_to_rgb(P(src), wm, h, P(want), want.strides[0], order, oa, uncl) == 0
    if gpu is None:
        return
    d = dev(before)
    gpu.yuv411_to_rgb(dev(src), d, wm, h, out_order=order, out_alpha=oa, unclamped=uncl)
    same_whole(host(d), want, before, h, "yuv411_to_rgb 3840x2160 order=%d alpha=%d unclamped=%d" % (order, oa, uncl))


YUV411_4K_CASES = [(0, 0, 0), (2, 1, 1)]


@G
@pytest.mark.parametrize("case", YUV411_4K_CASES, ids=lambda c: "k_yuv411_to_rgb-order%d-alpha%d-unclamped%d" % c)
def test_yuv411_to_rgb_4k(gpu, orc, case):
    """palette.hip k_yuv411_to_rgb: 2,073,600 macropixels against a grid capped at 8 workgroups of 256 threads per CU: every thread walks several cells"""
    run_yuv411_to_rgb_4k(orc, gpu, *case)


def run_clamp_switch_4k(orc, gpu, to_unclamped):
    w, h = 3840, 2160
    assert w * 4 * h > CAPS[("palette.hip", "k_clamp_switch")] * 256 * 16          # more than one pass of 4096 workgroups x 256 lanes x 16 bytes
    rng = seeded("clamp_4k", to_unclamped)
    plane = rng.integers(0, 256, (h + GUARD, w * 4), dtype=np.uint8)
    want = [plane.copy()]
    wp, ws = po.planes_args(want)
    assert orc.orc_switch_yuv_clamping(ctypes.addressof(wp), ctypes.addressof(ws), 589, h, to_unclamped) == 0
    if gpu is None:
        return
    d = dev(plane)
    gpu.yuv_switch_clamping([d], 589, h, to_unclamped)
    same_whole(host(d), want[0], plane, h, "switch clamping 3840x2160 to_unclamped=%d" % to_unclamped)


@G
@pytest.mark.parametrize("to_unclamped", [0, 1])
def test_clamp_switch_4k(gpu, orc, to_unclamped):
    """palette.hip k_clamp_switch: one YUVA8888 plane of 3840x2160 (33 MB; 4096 workgroups cover 16.7 MB per pass), both directions, guard rows behind the plane"""
    run_clamp_switch_4k(orc, gpu, to_unclamped)


# ---------------------------------------------------------------------------------------------- the oracle alone accepts every geometry (no GPU)
def _notune(name, value):
    raise AssertionError("the oracle-only pass must not touch the library")


ALL_CASES = ([(run_swizzle, c) for c in SWIZZLE_CASES] + [(run_gamma, c) for c in GAMMA_CASES] + [(run_premult, c) for c in PREMULT_CASES] + [(run_byte_luts, c) for c in BYTE_LUTS_CASES]
             + [(run_premult_yuva, c) for c in PREMULT_YUVA_CASES] + [(run_swizzle_batch, c) for c in SWIZZLE_BATCH_CASES] + [(run_pixel2, c) for c in PIXEL2_CASES]
             + [(run_mirror, c) for c in MIRROR_CASES] + [(run_letterbox, c) for c in LETTERBOX_CASES] + [(run_rgb_to_yuv, c) for c in K4_CASES]
             + [(run_rgb_to_yuv, (0, 1, 18, fmt, heights(S_K4, unit=2 if fmt == 4 else 1)[1], 3)) for fmt in (2, 4)] + [(run_yuv_to_rgb, c) for c in K3_CASES]
             + [(run_rgb_to_yuv411, c) for c in RGB411_CASES] + [(run_r411, c) for c in R411_CASES]
             + [(run_cup, c) for c in CUP_CASES] + [(run_rpk, c) for c in RPK_CASES]
             + [(run_yuv420p, c) for c in K2_CASES] + [(run_yuv420p_lut16, c) for c in K2_LUT16_CASES] + [(run_resize, c) for c in RESIZE_CASES] + [(run_gauss5, c) for c in GAUSS5_CASES]
             + [(run_composite, c) for c in COMPOSITE_CASES] + [(run_transition, c) for c in TRANSITION_CASES] + [(run_slide_over, c) for c in SLIDE_CASES]
             + [(run_triple_split, c) for c in SPLIT_CASES] + [(run_dissolve, c) for c in DISSOLVE_CASES] + [(run_deinterlace, c) for c in DEINT_CASES]
             + [(lambda orc, gpu, *c: run_edge(orc, gpu, _notune, *c), c) for c in EDGE_CASES] + [(lambda orc, gpu, *c: run_edge(orc, gpu, _notune, *c, quads=1), c) for c in EDGE4_CASES] + [(run_blurzoom, c) for c in BZ_CASES] + [(run_rgbdelay, c) for c in RGBD_CASES]
             + [(run_yuv411_to_rgb_4k, c) for c in YUV411_4K_CASES] + [(run_clamp_switch_4k, (t,)) for t in (0, 1)])


def test_oracle_accepts_every_geometry(orc):
    """every case of this module through the oracle alone: each orc_* call that reports a status returns 0 and none writes past its frame, so no GPU case can be
    lost to an oracle refusal -- a pair or shape the oracle declines does not belong in the lists above"""
    for fn, case in ALL_CASES:
        fn(orc, None, *case)
