"""Every row kernel on frames wider than one workgroup (strip, tile) and at every tail phase, bit for bit against the CPU oracle.

tests/test_tall_frames.py varies grid.y, tests/test_address_alignment.py the address bits, the plan tests of resize.hip and pixbuf.hip the dispatch.  This module
varies x: most vector forms give a lane 4 pixels and a workgroup kBlock = 256 lanes, so the second blockIdx.x of those kernels begins at pixel 1024 -- beyond every
width the other suites draw -- and their tails depend on width mod 4 (mod 8, mod 16 bytes), which five or six fixed sizes meet by luck only.

SPANS below is the table of launch sites whose grid.x (or strip, tile or linear-cell count) is derived from the width, in swizzle.hip, effects.hip, stencil.hip,
palette.hip, yuv.hip, fused.hip and runtime.hip.  Per site: the `unit` (pixels -- bytes where said -- one lane owns in x) and the `span` (what one workgroup, strip
or tile covers in x), both read from the kernels.  test_spans_match_the_sources (no GPU) scans the sources for row_grid / row_grid2 calls, cdiv(.., kBlock | 248 |
62u | 256u | kStW | kEmW), the `(cells + 511) / 512` walks and the quad walk of k_edge_paint4, and fails when a site is added, removed or changes its expression, so the widths cannot fall behind the code.

Out of scope: pixbuf.hip and resize.hip (tests/test_pixbuf_plans.py and tests/test_resize_plans.py pin gx, tiles_x, strips and cgroups per row) and the k_pb_half
callers of flat.hip (tests/test_pbh_row_step.py holds the strip seams).

widths() is the only place a width is computed.  With span S, unit u and the granularity g the entry point or the form demands:
  wide    the largest admissible width <= S (the first workgroup's last lane holds the tail); the smallest > S (the second workgroup gets one lane); the smallest > S
          that leaves a partial unit, where the form takes one; and the smallest admissible width >= 2 S + u + 1 with a non-zero tail (three workgroups, the last one
          partial).  Linear-cell kernels (512 lanes walk cells = ngr x rows): ngr = 511, 512, 513 and 2 x 512 + 1.
  narrow  every admissible width from the minimum tools/fuzz_ops.py draws for the kind (that bound is pinned to the live reference) up to 2 u + 1; for the cell
          kernels ngr = 1 and 2.
Phases that are not the total width (mirror axis, letterbox offset, gamma sub-rectangle, composite layers, split columns) have their own cases further down.

Heights are the smallest at which every row role occurs; the table says which and why.

A case compares like tests/test_tall_frames.py: inputs from tests.util.frame with row padding and two guard rows, the destination the fill byte (out of place) or
the source (in place), the oracle on a host copy, and same_whole() over the whole allocation.  Every case names the kernel form it expects and restates the
dispatcher's rule (the rule_* functions of tests/test_address_alignment.py) over its own pitches; with gpu=None (test_oracle_accepts_every_case) the inputs, the
oracle, the guard bytes and that restatement run without a device, and test_cases_reach_their_forms holds each group of cases to the FORMS it has to reach.
"""
import collections
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import test_address_alignment as ta
from tests import test_tall_frames as tt
from tests.test_tall_frames import FILL, GUARD, blank, ptrs, same_whole, seeded, src_frame
from tests.util import align, dev, frame, host

G = pytest.mark.gpu
P = po.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("swizzle.hip", "effects.hip", "stencil.hip", "palette.hip", "yuv.hip", "fused.hip", "runtime.hip")

# n: how often the expression occurs in the file; unit / span in pixels unless `what` says bytes; linear: a walk over cells = (width >> shift) x rows by
# workgroups of 512 (k_yuv420p_to_rgb_s: `block`) lanes, where span = lanes x unit; rows + why: the smallest height with every row role
Site = collections.namedtuple("Site", "n kernels unit span rows why linear")


def site(n, kernels, unit, span, rows=3, why="pointwise: first, inner and last row", linear=False):
    return Site(n, kernels, unit, span, rows, why, linear)


STENCIL3 = "3 x 3 neighbourhood: reach 1 + two rows beyond it on each side of an inner row"
SPANS = {
    ("swizzle.hip", "row_grid((width>>2)+1)"): site(1, "k_swizzle<IB,OB,LUT>", 4, 1024),
    ("swizzle.hip", "row_grid(width)"): site(3, "k_swizzle_bytes, k_premult<false>, k_premult_yuva<0>", 1, 256),
    ("swizzle.hip", "row_grid(chunks)"): site(1, "k_gamma_apply (bytes: a lane owns one 16-byte chunk)", 16, 4096),
    ("swizzle.hip", "row_grid((b1-b0))"): site(1, "k_gamma_apply_bytes (bytes)", 1, 256),
    ("swizzle.hip", "row_grid(((width+3)>>2))"): site(1, "k_premult<true>", 4, 1024),
    ("swizzle.hip", "row_grid(((width+3)/4))"): site(1, "k_byte_luts<PS>", 4, 1024),
    ("swizzle.hip", "row_grid(width/4)"): site(1, "k_premult_yuva<1>", 4, 1024),
    ("effects.hip", "row_grid2((width>>2)+1)"): site(1, "k_pixel2<PS,F>", 4, 1024),
    ("effects.hip", "row_grid2(width)"): site(2, "k_chroma_argb, k_mirror<PS>", 1, 256),
    ("effects.hip", "row_grid2(((width+3)>>2))"): site(1, "k_mirror_v4", 4, 1024, 4, "rows h - hh + 1 .. h - 1 are reflected: an even height with two rows on either side"),
    ("effects.hip", "row_grid2(((nwidth+3)>>2))"): site(2, "k_letterbox<PS>, k_letterbox_bars<PS>", 4, 1024, 5, "a bar row above, three inner rows, a bar row below"),
    ("effects.hip", "cdiv(owidth,kBlock)"): site(1, "k_composite<PS>", 1, 256, 5, "layers that begin above, inside and end below the frame"),
    ("effects.hip", "cdiv(half,kBlock)"): site(1, "k_transition<PS> (a lane owns two groups of 4 pixels, half a frame apart; groups run on from row to row, so S and S + 1 are nominal: at 5 rows every "
                                               "width from 409 pixels has a second workgroup, and the widths put workgroup boundaries and the half-frame seam inside rows)", 4, 1024, 5,
                                               "an odd number of rows: the two halves split a row"),
    ("effects.hip", "cdiv(width,kBlock)"): site(3, "k_slide_over<PS>, k_triple_split, k_dissolve<PS>", 1, 256),
    ("stencil.hip", "cdiv((width>>2),62u)"): site(1, "k_softlight_s<RB> (strips of 62 quads)", 4, 248, 4, STENCIL3 + "; even for the 4:2:0 planes"),
    ("stencil.hip", "cdiv(cp.w,256u)"): site(1, "k_softlight_s<RB>'s copy blocks (bytes of a copied plane: tiles of 256 columns, 16 bytes a lane; the grid is the wider of this and the strips)", 16, 256, 4,
                                             "as the strips"),
    ("stencil.hip", "cells(quads)/kBlock"): site(1, "k_edge_paint4 (quads of 4 pixels run on from row to row, a quad a lane; grid capped per CU, so S and S + 1 are nominal)", 4, 1024, 6,
                                                 "edge: the map's border of two rows and two inner rows"),
    ("stencil.hip", "cdiv(width,kStW)"): site(2, "k_softlight, k_edge_map<PS> (tiles of kStW = 64 columns)", 4, 64, 6, "edge: 5 x 5 reach 2 + two rows; softlight: " + STENCIL3),
    ("stencil.hip", "cdiv(width,kBlock)"): site(1, "k_edge_paint<PS>", 1, 256, 6, "edge: the map's border of two rows and two inner rows"),
    ("stencil.hip", "cdiv(width,kEmW)"): site(1, "k_edge_map4<TH> (tiles of kEmW = 128 columns)", 4, 128, 6, "edge: the map's border of two rows and two inner rows"),
    ("stencil.hip", "cdiv(vw,kBlock)"): site(1, "k_bz_update, k_bz_color", 1, 256, 6, "blurzoom: the blur leaves rows 0 and h - 1 out; an even height for the zoom's centre"),
    ("stencil.hip", "cdiv(bw,kBlock)"): site(1, "k_bz_blur, k_bz_zoom (the buffer: width rounded down to 32)", 1, 256, 6, "as k_bz_update"),
    ("stencil.hip", "cdiv(a.ntrip,kBlock)"): site(1, "k_deinterlace (a lane owns three pixels)", 3, 768, 6, "rows 0 and h - 1 are copied, two row pairs between them"),
    ("stencil.hip", "cdiv(wb,kBlock)"): site(1, "k_rgbd_snapshot (bytes)", 1, 256),
    ("stencil.hip", "cdiv(span,kBlock)"): site(1, "k_rgbdelay<SMALL>", 1, 256),
    ("stencil.hip", "cdiv(((orow+11)/12),kBlock)"): site(1, "k_rgbdelay4<SMALL> (12 bytes of the row and its padding)", 4, 1024),
    ("palette.hip", "cells(width>>2)/512:k_rgb_to_yuv420_s"): site(1, "k_rgb_to_yuv420_s<ORDER>", 4, 2048, 4, "4:2:0: row 0 alone, a row pair, the trailing row (and 6 rows: two pairs)", True),
    ("palette.hip", "cells(width>>2)/512:k_rgb_to_yuv422_s"): site(1, "k_rgb_to_yuv422_s<ORDER,FMT>", 4, 2048, linear=True),
    ("palette.hip", "cells(width>>2)/512:k_rgb_to_yuv444_s"): site(1, "k_rgb_to_yuv444_s<ORDER,IPS,AO,PLANAR>", 4, 2048, linear=True),
    ("palette.hip", "cdiv(npairs,kBlock)"): site(1, "k_rgb_to_yuv<ORDER,FMT> (a lane owns a pixel pair)", 2, 512, 4, "4:2:0 walks row pairs: two of them"),
    ("palette.hip", "cells(width>>2)/512:k_uyvy_to_rgb_s"): site(1, "k_uyvy_to_rgb_s", 4, 2048, linear=True),
    ("palette.hip", "cells(width>>2)/512:k_yuv444_to_rgb_s"): site(1, "k_yuv444_to_rgb_s", 4, 2048, linear=True),
    ("palette.hip", "cdiv(((width+1)>>1),kBlock)"): site(1, "k_yuv_to_rgb<FMT,ORDER>", 2, 512),
    ("palette.hip", "cdiv((width>>2),kBlock)"): site(2, "k_rgb_to_yuv411, k_yuv411_repack (a lane owns a macropixel)", 4, 1024, 4, "the 4:2:0 sides need an even height: two row pairs"),
    ("palette.hip", "cdiv(ncells,kBlock)"): site(1, "k_yuv411_to_rgb (macropixels run on from row to row; grid capped per CU)", 4, 1024),
    ("palette.hip", "cdiv(((n0+15)/16),kBlock)"): site(1, "k_clamp_switch (bytes of a whole plane, 16 per lane: rows and padding as one stream)", 16, 4096),
    ("palette.hip", "cdiv((width>>1),kBlock)"): site(1, "k_chroma_up_packed (a lane owns a pixel pair)", 2, 512, 4, "4:2:0: the first pair, an inner pair boundary, the last row"),
    ("palette.hip", "cells(width>>3)/512:k_420_to_packed_s"): site(1, "k_420_to_packed_s", 8, 4096, 4, "4:2:0 source: two row pairs", True),
    ("palette.hip", "cells(width>>2)/512:k_combine_s"): site(1, "k_combine_s", 4, 2048, linear=True),
    ("palette.hip", "cells(width>>2)/512:k_split_s"): site(1, "k_split_s", 4, 2048, linear=True),
    ("palette.hip", "cells(width>>3)/512:k_swab_s"): site(1, "k_swab_s", 8, 4096, linear=True),
    ("palette.hip", "cells(width>>3)/512:k_pk_to_s"): site(1, "k_pk_to_s<KIND>", 8, 4096, 4, "the 4:2:0 target walks row pairs: two of them", True),
    ("palette.hip", "cells(width>>2)/512:k_888_to_s"): site(1, "k_888_to_s<KIND>", 4, 2048, 4, "the 4:2:0 target walks row pairs: two of them", True),
    ("palette.hip", "cells(width>>3)/512:k_420_to_422p_s"): site(1, "k_420_to_422p_s", 8, 4096, 4, "4:2:0 source: two row pairs", True),
    ("palette.hip", "cdiv(((span+1)>>1),kBlock)"): site(1, "k_yuv_repack (a lane owns a pixel pair)", 2, 512, 4, "4:2:0 sides walk row pairs: two of them"),
    ("yuv.hip", "cdiv((width>>1),kBlock)"): site(1, "k_yuv420p_to_rgb, k_yuv422p_to_rgb (a lane owns a chroma column)", 2, 512, 6, "4:2:0: row 0 alone, two row pairs, the trailing row; and 5 rows: no trailing row"),
    ("yuv.hip", "cells(ncg)/s_block:k_yuv420p_to_rgb_s"): site(1, "k_yuv420p_to_rgb_s<NC,..> (a lane owns NC chroma columns; 512 lanes; NC = 2 unless tuned)", 4, 2048, 6, "as k_yuv420p_to_rgb", True),
    ("fused.hip", "cdiv(width,248)"): site(2, "k_gauss5_colorkey<PS> from lgpu_gauss5 and lgpu_gauss5_colorkey (a wave owns a strip of 62 quads, a workgroup four strips)", 4, 992, 9,
                                           "5 x 5 reach 2 + two rows, and a second band of 8 rows"),
    ("runtime.hip", "cdiv(nbytes,kBlock)"): site(1, "k_fill_pattern (bytes)", 1, 256),
}


# ---------------------------------------------------------------------------------------------- the table against the sources
DIVISORS = ("kBlock", "248", "62u", "256u", "kStW", "kEmW")


def squeeze(s):
    return re.sub(r"\s+|\(unsigned(?: long long)?\)|\blgpu::", "", s)


def call_args(text, start):
    """the top-level arguments of the call whose opening parenthesis ends at text[start - 1]; None when the line ends first"""
    depth, args, cur = 1, [], ""
    for ch in text[start:]:
        if ch == "(":
            depth += 1
        elif ch == ")":
            depth -= 1
            if depth == 0:
                return args + [cur]
        if ch == "," and depth == 1:
            args.append(cur)
            cur = ""
        else:
            cur += ch
    return None


def sites_in(lines):
    out, shift = [], None
    for n, line in enumerate(lines):
        m = re.search(r"\bngr\s*=\s*(?:a\.)?width\s*>>\s*(\d)", line)
        if m:
            shift = int(m.group(1))
        for m in re.finditer(r"\b(row_grid2?|cdiv)\(", line):
            a = call_args(line, m.end())
            if a is None or len(a) != 2 or re.match(r"\s*unsigned\b", a[0]):          # (a definition's parameter list is no call)
                continue
            a = [squeeze(x) for x in a]
            if m.group(1) != "cdiv":
                out.append("%s(%s)" % (m.group(1), a[0]))
            elif a[1] in DIVISORS and a[0] != "items_per_row":                            # (row_grid's own cdiv: the calls of row_grid are the sites)
                out.append("cdiv(%s,%s)" % tuple(a))
        if "dim3" in line and re.search(r"\+511\)/512", squeeze(line)):
            k = re.search(r"\bk_\w+", " ".join(lines[n:n + 4]))
            out.append("cells(width>>%s)/512:%s" % (shift, k.group(0) if k else "?"))
        if re.search(r"\(quads\+kBlock-1\)/kBlock", squeeze(line)):
            out.append("cells(quads)/kBlock")
        if re.search(r"\(cells\+s_block-1\)/s_block", squeeze(line)):
            k = re.search(r"\bk_\w+", " ".join(lines[n:n + 12]))
            out.append("cells(ncg)/s_block:%s" % (k.group(0) if k else "?"))
    return out


def scan_spans(root=ROOT):
    found = collections.Counter()
    for f in FILES:
        with open(os.path.join(root, "lives_amd", "csrc", f)) as fh:
            for s in sites_in(fh.read().split("\n")):
                found[(f, s)] += 1
    return found


def test_the_scan_reads_the_idioms():
    assert sites_in(["    const dim3 grid = with_frames(row_grid((unsigned)(width >> 2) + 1, height), n);"]) == ["row_grid((width>>2)+1)"]
    assert sites_in(["  dim3 g4 = row_grid2((unsigned)((width + 3) >> 2), height);"]) == ["row_grid2(((width+3)>>2))"]
    assert sites_in(["static inline dim3 row_grid(unsigned items_per_row, int height) {", "  return dim3(cdiv(items_per_row, kBlock), gy, 1);"]) == []
    assert sites_in(["  const dim3 vgrid(cdiv((unsigned)vw, kBlock), (unsigned)(vh < 1024 ? vh : 1024)), bgrid(cdiv((unsigned)bw, kBlock), (unsigned)(bh < 1024 ? bh : 1024));"]) == \
        ["cdiv(vw,kBlock)", "cdiv(bw,kBlock)"]
    assert sites_in(["  const unsigned strips = cdiv((unsigned)(width >> 2), 62u), bands = cdiv((unsigned)height, (unsigned)(4 * rb));"]) == ["cdiv((width>>2),62u)"]
    assert sites_in(["  a.strips = (int)cdiv((unsigned)width, 248); a.cgroups = (a.strips + 3) / 4;"]) == ["cdiv(width,248)"]
    assert sites_in(["    const unsigned nt4 = cdiv((unsigned)width, (unsigned)kEmW) * cdiv((unsigned)height, (unsigned)(eh == 16 ? 16 : 32));"]) == ["cdiv(width,kEmW)"]
    assert sites_in(["    const int ngr = width >> 3;", "    hipLaunchKernelGGL(lgpu::k_swab_s, dim3((unsigned)(((unsigned long long)ngr * height + 511) / 512)), dim3(512), 0, st, a, magic);"]) == \
        ["cells(width>>3)/512:k_swab_s"]
    assert sites_in(["  dim3 grid(lgpu::cdiv((unsigned)nbytes, lgpu::kBlock), (unsigned)(rows > 512 ? 512 : rows));"]) == ["cdiv(nbytes,kBlock)"]
    assert sites_in(["  const unsigned cx = cdiv((unsigned)cp.w, 256u), cy = cdiv((unsigned)cp.h, 16u);"]) == ["cdiv(cp.w,256u)"]
    assert sites_in(["      const unsigned pcap = (unsigned)device_cus() * 8u, pneed = (unsigned)((quads + kBlock - 1) / kBlock);"]) == ["cells(quads)/kBlock"]


def test_spans_match_the_sources():
    """every row_grid / row_grid2 call, every cdiv by kBlock, 248, 62u, 256u, kStW or kEmW, every 512-lane cell walk and the quad walk of the seven files, per file and expression -- and how
    often: a new launch site, a removed one or a changed expression fails here until SPANS (and with it the widths of this module) follows"""
    want = collections.Counter({k: v.n for k, v in SPANS.items()})
    found = scan_spans()
    assert found == want, "x launch sites in the sources and SPANS of tests/test_wide_frames.py differ: only in the sources %s, only in SPANS %s -- update SPANS (unit and span from the kernel) and the cases of the site" % (
        dict(found - want), dict(want - found))
    with open(os.path.join(ROOT, "lives_amd", "csrc", "lgpu_common.h")) as f:
        assert re.search(r"constexpr int kBlock = 256;", f.read()), "kBlock changed: every span of SPANS is a multiple of it"
    with open(os.path.join(ROOT, "lives_amd", "csrc", "stencil.hip")) as f:
        text = f.read()
    assert re.search(r"constexpr int kStW = 64\b", text) and re.search(r"constexpr int kEmW = 128\b", text), "a tile width of stencil.hip changed: SPANS records 64 and 128"


# ---------------------------------------------------------------------------------------------- widths
ASKED = set()          # the sites widths() was asked for


def widths(key, g=1, lo=1, partial=True, unit=None, span=None):
    """(wide, narrow) for a launch site; g: the granularity of admissible widths, lo: the smallest width the kind is defined for; unit / span override the table's where
    the table counts bytes and the caller pixels"""
    e = SPANS[key]
    ASKED.add(key)
    u, S = unit or e.unit, span or e.span
    up = lambda n: -(-n // g) * g
    lo = up(lo)
    if e.linear:                  # cells of u pixels: the cell forms take whole cells only unless the caller says otherwise (g), and ngr = 1 and 2 are the narrow sweep
        g = g if g > 1 else u
        return [u * n for n in (511, 512, 513, 2 * 512 + 1)], list(range(up(max(lo, g)), 2 * u + 2, g))
    tail = lambda w: partial and u > 1 and g % u != 0 and w % u == 0           # a width without the partial unit the form could take
    wide = [S // g * g, up(S + 1)]
    w = up(S + 1)
    while tail(w):
        w += g
    if w not in wide:
        wide.append(w)
    w = up(2 * S + u + 1)
    while tail(w):
        w += g
    wide.append(w)
    return wide, list(range(lo, 2 * u + 2, g))


def both(key, **kw):
    wide, narrow = widths(key, **kw)
    return narrow + wide


def test_widths():
    assert widths(("swizzle.hip", "row_grid((width>>2)+1)")) == ([1024, 1025, 2053], [1, 2, 3, 4, 5, 6, 7, 8, 9])
    assert widths(("swizzle.hip", "row_grid(width/4)"), g=4, lo=4) == ([1024, 1028, 2056], [4, 8])
    assert widths(("swizzle.hip", "row_grid(width)")) == ([256, 257, 514], [1, 2, 3])
    assert widths(("palette.hip", "cdiv(npairs,kBlock)"), g=2, lo=2) == ([512, 514, 1028], [2, 4])
    assert widths(("palette.hip", "cells(width>>3)/512:k_swab_s")) == ([4088, 4096, 4104, 8200], [8, 16])
    assert widths(("stencil.hip", "cdiv(a.ntrip,kBlock)")) == ([768, 769, 1540], [1, 2, 3, 4, 5, 6, 7])
    assert widths(("stencil.hip", "cdiv(width,kStW)"), lo=3)[0] == [64, 65, 133]


def pitch(w, ps, form):
    """form "v": 32-byte aligned rows with padding (every vector form); form "b": a pitch no vector form takes -- odd for 1- and 3-byte pixels, a multiple of 4 that is no multiple
    of 16 for 4-byte pixels (the entry points demand 4)"""
    if form == "v":
        return align(w * ps + 16, 32)
    n = w * ps + ps
    if ps == 4:
        return n if n & 15 else n + 4
    return n | 1


def kept(h, *pairs):
    """(the oracle's buffer, what it started as) pairs: the oracle left the guard rows behind the frame's h rows alone.  Every runner asserts it before it looks at `gpu`,
    so the pass without a device holds the oracle to it at every width of this module"""
    for want, before in pairs:
        assert (want[h:] == before[h:]).all(), "the oracle wrote past the frame's %d rows" % h


# ---------------------------------------------------------------------------------------------- the cases
# (group, expected form, run function, arguments); a run function is called as fn(orc, gpu, tune, form, *args) and asserts that the dispatcher's restated rule gives `form`
CASES = []
FORMS = {}


def add(group, form, fn, *args):
    CASES.append((group, form, fn, args))


def case_id(c):
    return "%s-%s-%s" % (c[0], re.sub(r"[^\w<>,+]+", "_", c[1]), "-".join(re.sub(r"[^\w.]+", "_", str(a)) for a in c[3]))


# ---- swizzle.hip
K_SWZ, K_ROW, K_GAM, K_GAMB = ("swizzle.hip", "row_grid((width>>2)+1)"), ("swizzle.hip", "row_grid(width)"), ("swizzle.hip", "row_grid(chunks)"), ("swizzle.hip", "row_grid((b1-b0))")
K_PRE, K_LUTS, K_PYUVA = ("swizzle.hip", "row_grid(((width+3)>>2))"), ("swizzle.hip", "row_grid(((width+3)/4))"), ("swizzle.hip", "row_grid(width/4)")
H3 = SPANS[K_SWZ].rows


def run_swizzle(orc, gpu, tune, form, opname, pf, w, use_lut, n=1):
    op = po.OPS.index(opname)
    ib, ob, h = po.OP_IBPP[op], po.OP_OBPP[op], H3
    rng = seeded("swizzle", opname, pf, w, use_lut, n)
    lut = rng.integers(0, 256, 256, dtype=np.uint8) if use_lut else None
    srcs = [src_frame(rng, w, h, ib, pitch(w, ib, pf)) for _ in range(n)]
    before = blank(h, pitch(w, ob, pf))
    assert ta.rule_swizzle(ib, ob, srcs[0].strides[0], before.strides[0]) == form
    wants = []
    for s in srcs:
        wt = before.copy()
        orc.orc_swizzle(op, 0, P(s), s.strides[0], P(wt), wt.strides[0], w, h, P(lut))
        wants.append(wt)
    wip = None
    if ib == ob and n == 1:
        wip = srcs[0].copy()
        orc.orc_swizzle(op, 0, P(wip), wip.strides[0], P(wip), wip.strides[0], w, h, P(lut))
    kept(h, *[(wt, before) for wt in wants] + ([(wip, srcs[0])] if wip is not None else []))
    if gpu is None:
        return
    what = "swizzle %s %s width %d lut=%d" % (opname, pf, w, use_lut)
    if n > 1:
        d_s, d_o = [dev(s) for s in srcs], [dev(before) for _ in range(n)]
        gpu.lib.call("lgpu_swizzle_batch", op, 0, ptrs(d_s), srcs[0].strides[0], ptrs(d_o), before.strides[0], w, h, lut.ctypes.data if use_lut else None, n, None)
        for f in range(n):
            same_whole(host(d_o[f]), wants[f], before, h, what + " batch frame %d" % f)
        return
    d = dev(before)
    gpu.swizzle(op, dev(srcs[0]), d, w, h, lut=lut)
    same_whole(host(d), wants[0], before, h, what)
    if wip is not None:
        d = dev(srcs[0])
        gpu.swizzle(op, d, d, w, h, lut=lut)
        same_whole(host(d), wip, srcs[0], h, what + " in place")


SWZ_OPS = ("swap3", "swap3addpost", "delpost", "swap3postalpha")
for _op in SWZ_OPS:
    _i = po.OPS.index(_op)
    for _w in both(K_SWZ):
        add("swizzle", "k_swizzle<%d,%d>" % (po.OP_IBPP[_i], po.OP_OBPP[_i]), run_swizzle, _op, "v", _w, _w & 1)
    for _w in both(K_ROW):
        add("swizzle", "k_swizzle_bytes", run_swizzle, _op, "b", _w, (_w >> 1) & 1)
add("swizzle", "k_swizzle<3,4>", run_swizzle, "swap3addpost", "v", widths(K_SWZ)[0][1], 1, 3)
add("swizzle", "k_swizzle_bytes", run_swizzle, "swap3postalpha", "b", widths(K_ROW)[0][1], 0, 3)
FORMS["swizzle"] = {"k_swizzle<3,3>", "k_swizzle<3,4>", "k_swizzle<4,3>", "k_swizzle<4,4>", "k_swizzle_bytes"}


def run_gamma(orc, gpu, tune, form, ps, af, pf, w, x=0, rw=None, n=1):
    """lgpu_gamma_apply on the rectangle of columns x .. x + rw - 1 and rows 1 .. h - 2 (the whole frame when rw is None), in place as the entry point is"""
    h = H3 if rw is None else H3 + 2
    y, rh = (0, h) if rw is None else (1, h - 2)
    rw = w if rw is None else rw
    rng = seeded("gamma", ps, af, pf, w, x, rw, n)
    lut = rng.integers(0, 256, 256, dtype=np.uint8)
    pix = [src_frame(rng, w, h, ps, pitch(w, ps, pf)) for _ in range(n)]
    rs = pix[0].strides[0]
    assert ta.rule_bits16(rs | (y * rs), "k_gamma_apply", "k_gamma_apply_bytes") == form
    wants = [a.copy() for a in pix]
    for a in wants:
        orc.orc_gamma_apply(a[y:, x * ps:].ctypes.data, rs, rw, rh, ps, af, P(lut))
    kept(h, *zip(wants, pix))
    if gpu is None:
        return
    what = "gamma ps=%d af=%d %s width %d rect x=%d w=%d" % (ps, af, pf, w, x, rw)
    ds = [dev(a) for a in pix]
    if n > 1:
        gpu.lib.call("lgpu_gamma_apply_batch", ptrs(ds), rs, x, y, rw, rh, ps, af, lut.ctypes.data, n, None)
    else:
        gpu.gamma_apply(ds[0], rw, rh, ps, lut, alpha_first=af, x=x, y=y)
    for f in range(n):
        same_whole(host(ds[f]), wants[f], pix[f], h, what + " frame %d" % f)


for _ps, _af in ((3, 0), (4, 0), (4, 1)):
    # the table counts bytes: pixels of _ps bytes are admissible every _ps bytes
    for _b in both(K_GAM, g=_ps, lo=_ps):
        add("gamma", "k_gamma_apply", run_gamma, _ps, _af, "v", _b // _ps)
    for _b in both(K_GAMB, g=_ps, lo=_ps):
        add("gamma", "k_gamma_apply_bytes", run_gamma, _ps, _af, "b", _b // _ps)
# sub-rectangles of 3-byte pixels: b0 = 3 x and b1 = 3 (x + 22) take every residue mod 16 (3 is a unit mod 16) over x = 0 .. 15
for _x in range(16):
    add("gamma", "k_gamma_apply", run_gamma, 3, 0, "v", 16 + 22 + 3, _x, 22)
for _x in range(4):
    add("gamma", "k_gamma_apply", run_gamma, 4, _x & 1, "v", 4 + 9 + 3, _x, 9 - _x)
# ... and rectangles across the boundary between the first two workgroups (byte 4096 of the 16-byte chunks that begin at b0 & ~15; byte b0 + 256 of the byte form)
_S = SPANS[K_GAM].span
add("gamma", "k_gamma_apply", run_gamma, 3, 0, "v", _S // 3 + 40, 7, _S // 3 + 11)
add("gamma", "k_gamma_apply", run_gamma, 4, 1, "v", _S // 4 + 40, 5, _S // 4 + 9)
add("gamma", "k_gamma_apply_bytes", run_gamma, 3, 0, "b", SPANS[K_GAMB].span // 3 + 40, 7, SPANS[K_GAMB].span // 3 + 11)
add("gamma", "k_gamma_apply", run_gamma, 4, 0, "v", widths(K_GAM, g=4, lo=4)[0][1] // 4, 0, None, 3)
FORMS["gamma"] = {"k_gamma_apply", "k_gamma_apply_bytes"}


def run_premult(orc, gpu, tune, form, af, un, pf, w, n=1):
    h = H3
    rng = seeded("premult", af, un, pf, w, n)
    pix = [frame(rng, w, h, 4, stride=pitch(w, 4, pf), extra_rows=GUARD, alpha_mix=True) for _ in range(n)]
    assert ta.rule_bits16(pix[0].strides[0], "k_premult<true>", "k_premult<false>") == form
    wants = [a.copy() for a in pix]
    for a in wants:
        orc.orc_alpha_premult(P(a), a.strides[0], w, h, af, un)
    kept(h, *zip(wants, pix))
    if gpu is None:
        return
    ds = [dev(a) for a in pix]
    if n > 1:
        gpu.lib.call("lgpu_alpha_premult_batch", ptrs(ds), pix[0].strides[0], w, h, af, un, n, None)
    else:
        gpu.alpha_premult(ds[0], w, h, alpha_first=af, un=un)
    for f in range(n):
        same_whole(host(ds[f]), wants[f], pix[f], h, "premult af=%d un=%d %s width %d frame %d" % (af, un, pf, w, f))


for _w in both(K_PRE):
    add("premult", "k_premult<true>", run_premult, _w & 1, (_w >> 1) & 1, "v", _w)
for _w in both(K_ROW):
    add("premult", "k_premult<false>", run_premult, _w & 1, (_w >> 1) & 1, "b", _w)
add("premult", "k_premult<true>", run_premult, 1, 0, "v", widths(K_PRE)[0][1], 3)
FORMS["premult"] = {"k_premult<true>", "k_premult<false>"}


def run_byte_luts(orc, gpu, tune, form, ps, pf, w):
    h = H3
    rng = seeded("byte_luts", ps, pf, w)
    luts = rng.integers(0, 256, (ps, 256), dtype=np.uint8)
    src = src_frame(rng, w, h, ps, pitch(w, ps, pf))
    before = blank(h, src.strides[0])
    assert form == "k_byte_luts<%d>" % ps            # one kernel per pixel size; the placement decides between its 16-byte and its byte-wise branch
    want, wip = before.copy(), src.copy()
    orc.orc_byte_luts(P(src), src.strides[0], P(want), want.strides[0], w, h, ps, luts.ctypes.data)
    orc.orc_byte_luts(P(wip), wip.strides[0], P(wip), wip.strides[0], w, h, ps, luts.ctypes.data)
    kept(h, (want, before), (wip, src))
    if gpu is None:
        return
    d = dev(before)
    gpu.byte_luts(dev(src), d, w, h, ps, luts)
    same_whole(host(d), want, before, h, "byte_luts ps=%d %s width %d" % (ps, pf, w))
    d = dev(src)
    gpu.byte_luts(d, d, w, h, ps, luts)
    same_whole(host(d), wip, src, h, "byte_luts ps=%d %s width %d in place" % (ps, pf, w))


for _ps in (3, 4):
    for _pf in "vb":
        for _w in both(K_LUTS):
            add("byte_luts", "k_byte_luts<%d>" % _ps, run_byte_luts, _ps, _pf, _w)
FORMS["byte_luts"] = {"k_byte_luts<3>", "k_byte_luts<4>"}


def run_premult_yuva(orc, gpu, tune, form, pal, clamped, un, pf, w):
    h = H3
    rng = seeded("premult_yuva", pal, clamped, un, pf, w)
    planes = [src_frame(rng, w, h, 4, pitch(w, 4, pf))] if pal == 589 else [src_frame(rng, w, h, 1, pitch(w, 1, pf)) for _ in range(4)]
    assert ("k_premult_yuva<1>" if clamped and pal == 589 and (w & 3) == 0 and (planes[0].strides[0] & 15) == 0 else "k_premult_yuva<0>") == form
    want = [p.copy() for p in planes]
    pp = (ctypes.c_void_p * 4)(*([x.ctypes.data for x in want] + [None] * (4 - len(want))))
    ss = (ctypes.c_int * 4)(*([x.strides[0] for x in want] + [0] * (4 - len(want))))
    orc.orc_alpha_premult_yuva(pp, ss, w, h, pal, clamped, un)
    kept(h, *zip(want, planes))
    if gpu is None:
        return
    ds = [dev(p) for p in planes]
    gpu.alpha_premult_yuva(ds, w, h, pal, clamped, un=un)
    for i in range(len(planes)):
        same_whole(host(ds[i]), want[i], planes[i], h, "premult yuva pal=%d clamped=%d un=%d %s width %d plane %d" % (pal, clamped, un, pf, w, i))


for _w in both(K_PYUVA, g=4, lo=4):
    add("premult_yuva", "k_premult_yuva<1>", run_premult_yuva, 589, 1, (_w >> 2) & 1, "v", _w)
for _w in both(K_ROW):
    # one pixel per lane: unclamped or planar layers, packed layers off 16-byte rows, and clamped packed layers whose width is no multiple of 4
    add("premult_yuva", "k_premult_yuva<0>", run_premult_yuva, 589, 0, _w & 1, "v", _w)
    add("premult_yuva", "k_premult_yuva<0>", run_premult_yuva, 589, 1, _w & 1, "b", _w)
    add("premult_yuva", "k_premult_yuva<0>", run_premult_yuva, 545, (_w >> 1) & 1, _w & 1, "b", _w)
    if _w & 3:
        add("premult_yuva", "k_premult_yuva<0>", run_premult_yuva, 589, 1, _w & 1, "v", _w)
FORMS["premult_yuva"] = {"k_premult_yuva<1>", "k_premult_yuva<0>"}


# ---- effects.hip
K_PIX2, K_ROW2, K_MIR4, K_LBOX = ("effects.hip", "row_grid2((width>>2)+1)"), ("effects.hip", "row_grid2(width)"), ("effects.hip", "row_grid2(((width+3)>>2))"), ("effects.hip", "row_grid2(((nwidth+3)>>2))")
K_COMP, K_TRANS, K_COL = ("effects.hip", "cdiv(owidth,kBlock)"), ("effects.hip", "cdiv(half,kBlock)"), ("effects.hip", "cdiv(width,kBlock)")


def run_pixel2(orc, gpu, tune, form, kind, ps, extra, pf, w, n=1):
    """lgpu_blend_chroma (extra: alpha first) / _luma (extra: type) / _multi (extra: type) / lgpu_colorkey; n > 1: lgpu_colorkey_batch, or lgpu_fx_batch for the blends"""
    h, bf = H3, 100
    rng = seeded("pixel2", kind, ps, extra, pf, w, n)
    st = pitch(w, ps, pf)
    s1 = [frame(rng, w, h, ps, stride=st, extra_rows=GUARD, alpha_mix=True) for _ in range(n)]
    s2 = [frame(rng, w, h, ps, stride=st, extra_rows=GUARD, alpha_mix=True) for _ in range(n)]
    before = blank(h, st)
    assert ta.rule_pixel2(ps, st, argb=(kind == "chroma" and ps == 4 and extra)) == form

    def oracle(a, b, out, inplace):
        if kind == "chroma":
            orc.orc_blend_chroma(P(a), st, P(b), st, P(out), st, w, h, ps, extra, bf)
        elif kind == "luma":
            orc.orc_blend_luma(extra, P(a), st, P(b), st, P(out), st, w, h, ps, 0, bf, inplace)
        elif kind == "multi":
            orc.orc_blend_multi(extra, P(a), st, P(b), st, P(out), st, w, h, 0, bf)
        else:
            orc.orc_colorkey(P(a), st, P(b), st, P(out), st, w, h, 0, 0.35, 0.7, 40, 200, 90, 0)

    def launch(d1, d2, dd):
        if kind == "chroma":
            gpu.blend_chroma(d1, d2, dd, w, h, ps, bf, alpha_first=extra)
        elif kind == "luma":
            gpu.blend_luma(extra, d1, d2, dd, w, h, ps, 0, bf)
        elif kind == "multi":
            gpu.blend_multi(extra, d1, d2, dd, w, h, 0, bf)
        else:
            gpu.colorkey(d1, d2, dd, w, h, 0, 0.35, 0.7, (40, 200, 90))

    wants = []
    for f in range(n):
        wt = before.copy()
        oracle(s1[f], s2[f], wt, 0)
        wants.append(wt)
    wip = s1[0].copy()
    oracle(wip, s2[0], wip, 1)
    kept(h, *[(wt, before) for wt in wants] + [(wip, s1[0])])
    if gpu is None:
        return
    what = "%s ps=%d %s %s width %d" % (kind, ps, extra, pf, w)
    if n > 1:
        d1, d2, dd = [dev(a) for a in s1], [dev(a) for a in s2], [dev(before) for _ in range(n)]
        if kind == "colorkey":
            gpu.lib.call("lgpu_colorkey_batch", ptrs(d1), st, ptrs(d2), st, ptrs(dd), st, w, h, 0, 0.35, 0.7, 40, 200, 90, n, None)
        else:
            ip = {"chroma": (ps, 0), "luma": (extra, ps, 0), "multi": (extra, 0)}[kind]
            gpu.fx_batch(ta.FX[kind], [[t] for t in d1], [[t] for t in dd], w, h, ins1=[[t] for t in d2], ip=ip, dp=(float(bf),))
        for f in range(n):
            same_whole(host(dd[f]), wants[f], before, h, what + " batch frame %d" % f)
        return
    d = dev(before)
    launch(dev(s1[0]), dev(s2[0]), d)
    same_whole(host(d), wants[0], before, h, what)
    d = dev(s1[0])
    launch(d, dev(s2[0]), d)
    same_whole(host(d), wip, s1[0], h, what + " in place")


PIXEL2_KINDS = (("chroma", 3, 0), ("chroma", 4, 0), ("luma", 3, 1), ("luma", 4, 3), ("multi", 3, 5), ("colorkey", 3, 0))
for _kind, _ps, _extra in PIXEL2_KINDS:
    for _w in both(K_PIX2):
        add("pixel2", "k_pixel2<%d> vec" % _ps, run_pixel2, _kind, _ps, _extra, "v", _w)
        add("pixel2", "k_pixel2<%d> bytes" % _ps, run_pixel2, _kind, _ps, _extra, "b", _w)
for _w in both(K_ROW2):
    add("pixel2", "k_chroma_argb", run_pixel2, "chroma", 4, 1, "v", _w)
    add("pixel2", "k_chroma_argb", run_pixel2, "chroma", 4, 1, "b", _w)
for _kind, _ps, _extra in (("colorkey", 3, 0), ("chroma", 4, 0), ("luma", 3, 2), ("multi", 3, 1)):
    add("pixel2", "k_pixel2<%d> vec" % _ps, run_pixel2, _kind, _ps, _extra, "v", widths(K_PIX2)[0][1], 3)
FORMS["pixel2"] = {"k_pixel2<3> vec", "k_pixel2<3> bytes", "k_pixel2<4> vec", "k_pixel2<4> bytes", "k_chroma_argb"}


def mirror_branches(w, mx):
    """which branch of k_mirror_v4 each group of four pixels of a row takes: the kernel's conditions, restated"""
    hw, out = w >> 1, set()
    for x0 in range(0, w, 4):
        whole = x0 + 4 <= w
        if whole and (not mx or x0 + 3 <= hw):
            out.add("plain")
        elif whole and mx and x0 > hw:
            out.add("flipped")
        else:
            out.add("mixed" if whole else "partial")
    return out


def run_mirror(orc, gpu, tune, form, mode, ps, pf, w, n=1):
    h = SPANS[K_MIR4].rows
    rng = seeded("mirror", mode, ps, pf, w, n)
    st = pitch(w, ps, pf)
    srcs = [src_frame(rng, w, h, ps, st) for _ in range(n)]
    before = blank(h, st)
    assert ta.rule_mirror(ps, st) == form
    wants = []
    for s in srcs:
        wt = before.copy()
        orc.orc_mirror(mode, P(s), st, P(wt), st, w, h, ps)
        wants.append(wt)
    wip = srcs[0].copy()
    orc.orc_mirror(mode, P(wip), st, P(wip), st, w, h, ps)
    kept(h, *[(wt, before) for wt in wants] + [(wip, srcs[0])])
    if gpu is None:
        return
    what = "mirror mode=%d ps=%d %s width %d" % (mode, ps, pf, w)
    if n > 1:
        d_s, d_o = [dev(s) for s in srcs], [dev(before) for _ in range(n)]
        gpu.lib.call("lgpu_mirror_batch", mode, ptrs(d_s), st, ptrs(d_o), st, w, h, ps, n, None)
        for f in range(n):
            same_whole(host(d_o[f]), wants[f], before, h, what + " batch frame %d" % f)
        return
    d = dev(before)
    gpu.mirror(mode, dev(srcs[0]), d, w, h, ps)
    same_whole(host(d), wants[0], before, h, what)
    d = dev(srcs[0])
    gpu.mirror(mode, d, d, w, h, ps)
    same_whole(host(d), wip, srcs[0], h, what + " in place")


# hw = width >> 1 at every residue mod 4, beyond the first workgroup: S + 1, S + 3, S + 5, S + 7
MIRROR_AXIS = [SPANS[K_MIR4].span + 2 * r + 1 for r in range(4)]
for _mode in (0, 1, 2):
    for _w in sorted(set(both(K_MIR4) + (MIRROR_AXIS if _mode != 1 else []))):
        add("mirror", "k_mirror_v4", run_mirror, _mode, 4, "v", _w)
    for _w in both(K_ROW2):
        add("mirror", "k_mirror<4>", run_mirror, _mode, 4, "b", _w)
        add("mirror", "k_mirror<3>", run_mirror, _mode, 3, "bv"[_w & 1], _w)
add("mirror", "k_mirror_v4", run_mirror, 2, 4, "v", MIRROR_AXIS[1], 3)
add("mirror", "k_mirror<3>", run_mirror, 0, 3, "v", widths(K_ROW2)[0][1], 3)
FORMS["mirror"] = {"k_mirror_v4", "k_mirror<3>", "k_mirror<4>"}


def test_mirror_cases_enter_every_branch():
    """the x and xy cases of k_mirror_v4 put hw = width >> 1 at all four residues mod 4, and each branch of the kernel (plain, flipped, mixed, partial last group) is
    entered by one case at least -- below the workgroup boundary and beyond it"""
    ws = sorted({c[3][3] for c in CASES if c[0] == "mirror" and c[1] == "k_mirror_v4" and c[3][0] in (0, 2)})
    S = SPANS[K_MIR4].span
    for sel, name in ((lambda w: w <= S, "up to"), (lambda w: w > S, "beyond")):
        sub = [w for w in ws if sel(w)]
        assert {(w >> 1) & 3 for w in sub} == {0, 1, 2, 3}, "%s %d pixels: hw residues %s" % (name, S, sorted({(w >> 1) & 3 for w in sub}))
        reached = set().union(*[mirror_branches(w, 1) for w in sub])
        assert reached == {"plain", "flipped", "mixed", "partial"}, "%s %d pixels the cases reach only %s" % (name, S, sorted(reached))
    assert mirror_branches(8, 1) == {"plain", "mixed"} and mirror_branches(11, 1) == {"plain", "mixed", "partial"} and mirror_branches(16, 0) == {"plain"}
    assert mirror_branches(16, 1) == {"plain", "mixed", "flipped"}


BLACK = tt.BLACK


def run_letterbox(orc, gpu, tune, form, ps, pf, ox, w, entry, n=1):
    """a frame of w x 3 centred on a canvas of (w + 2 ox) x 5, so that the centred entry points and lgpu_letterbox_at / lgpu_letterbox_bars at (ox, 1) mean the same;
    entry: "centred" (lgpu_letterbox, or lgpu_letterbox_batch for n > 1), "at", "bars" (in place on a canvas that already holds the inner frame)"""
    nh = SPANS[K_LBOX].rows
    h, nw = nh - 2, w + 2 * ox
    oy = (nh - h + 1) >> 1
    assert (nw - w + 1) >> 1 == ox and oy == 1
    rng = seeded("letterbox", ps, pf, ox, w, entry, n)
    srcs = [src_frame(rng, w, h, ps, pitch(w, ps, pf)) for _ in range(n)]
    before = blank(nh, pitch(nw, ps, pf))
    bp = np.array(BLACK[ps], np.uint8)
    rule = ta.rule_letterbox(ps, srcs[0].strides[0], before.strides[0]) if entry != "bars" else "k_letterbox_bars<%d>" % ps
    assert rule == form
    wants = []
    for s in srcs:
        wt = before.copy()
        orc.orc_letterbox(P(s), s.strides[0], w, h, P(wt), wt.strides[0], nw, nh, ps, P(bp))
        wants.append(wt)
    canvas = src_frame(rng, nw, nh, ps, before.strides[0])
    wbars = canvas.copy()
    wbars[:nh, :nw * ps] = wants[0][:nh, :nw * ps]
    wbars[oy:oy + h, ox * ps:(ox + w) * ps] = canvas[oy:oy + h, ox * ps:(ox + w) * ps]
    kept(nh, *[(wt, before) for wt in wants] + [(wbars, canvas)])
    if gpu is None:
        return
    what = "letterbox %s ps=%d %s ox=%d width %d on %d" % (entry, ps, pf, ox, w, nw)
    black = (ctypes.c_uint8 * 4)(*BLACK[ps])
    if entry == "bars":
        d = dev(canvas)
        gpu.lib.call("lgpu_letterbox_bars", d.data_ptr(), d.stride(0), nw, nh, ps, black, ox, oy, w, h, None)
        same_whole(host(d), wbars, canvas, nh, what)
        return
    d_s, d_o = [dev(s) for s in srcs], [dev(before) for _ in range(n)]
    if n > 1:
        gpu.lib.call("lgpu_letterbox_batch", ptrs(d_s), srcs[0].strides[0], w, h, ptrs(d_o), before.strides[0], nw, nh, ps, black, n, None)
    elif entry == "at":
        gpu.lib.call("lgpu_letterbox_at", d_s[0].data_ptr(), d_s[0].stride(0), w, h, d_o[0].data_ptr(), d_o[0].stride(0), nw, nh, ps, black, ox, oy, None)
    else:
        gpu.letterbox(d_s[0], d_o[0], w, h, nw, nh, ps, BLACK[ps])
    for f in range(n):
        same_whole(host(d_o[f]), wants[f], before, nh, what + " frame %d" % f)


def lbox_form(ps, pf, entry):
    return "k_letterbox_bars<%d>" % ps if entry == "bars" else "k_letterbox<4> vec" if (ps == 4 and pf == "v") else "k_letterbox<%d>" % ps


_u, _S = SPANS[K_LBOX].unit, SPANS[K_LBOX].span
for _entry in ("centred", "at", "bars"):
    # every (ox mod 4, inner width mod 4) on a canvas of five to seven groups: ox = u + a, width = 2 u + b
    for _a in range(_u):
        for _b in range(_u):
            _ps, _pf = ((4, "v"), (3, "v"), (4, "b"), (1, "b"))[(_a + _b) & 3]
            add("letterbox", lbox_form(_ps, _pf, _entry), run_letterbox, _ps, _pf, _u + _a, 2 * _u + _b, _entry)
    # the canvas widths of the site (the inner frame two pixels in from either side), and a canvas beyond S whose inner frame crosses the workgroup boundary
    for _ps, _pf in ((4, "v"), (3, "b"), (1, "v"), (4, "b")):
        for _nw in widths(K_LBOX, lo=5)[0]:
            add("letterbox", lbox_form(_ps, _pf, _entry), run_letterbox, _ps, _pf, 2, _nw - 4, _entry)
        add("letterbox", lbox_form(_ps, _pf, _entry), run_letterbox, _ps, _pf, 2 * _u + 1, _S + 67 - 2 * (2 * _u + 1), _entry)
add("letterbox", "k_letterbox<4> vec", run_letterbox, 4, "v", 2, widths(K_LBOX)[0][1] - 4, "centred", 3)
add("letterbox", "k_letterbox<3>", run_letterbox, 3, "b", 3, widths(K_LBOX)[0][1] - 6, "centred", 3)
FORMS["letterbox"] = {"k_letterbox<1>", "k_letterbox<3>", "k_letterbox<4>", "k_letterbox<4> vec", "k_letterbox_bars<1>", "k_letterbox_bars<3>", "k_letterbox_bars<4>"}


def run_composite(orc, gpu, tune, form, ps, is_bgr, revz, ow):
    oh, S = SPANS[K_COMP].rows, SPANS[K_COMP].span
    rng = seeded("composite", ps, is_bgr, revz, ow)
    # (width, height, offs_x, offs_y, alpha): across the left edge and the top; left edge in the second workgroup; right edge in the second workgroup (it begins in the
    # first); entirely inside the second workgroup; and one across the right edge and the bottom of the frame
    geo = [(12, 3, -3, -1, 0.7312), (40, 3, S + 5, 1, 1.0), (S // 2 + 17, 2, S // 2, 2, 0.5), (10, 4, S + 30, 0, 0.25), (30, 3, ow - 9, oh - 2, 0.6)]
    geo = [g for g in geo if g[2] < ow]
    if ow > S + 45:
        assert geo[1][2] > S and geo[1][2] + geo[1][0] <= ow and geo[2][2] < S < geo[2][2] + geo[2][0] <= ow and geo[3][2] > S and geo[3][2] + geo[3][0] <= ow
    layers = [(src_frame(rng, w, h, ps, align(w * ps)), w, h, ox, oy, al) for (w, h, ox, oy, al) in geo]
    bg = [int(v) for v in rng.integers(0, 256, 3)]
    L = (po.CompLayer * len(layers))()
    for z, (a, w, h, ox, oy, al) in enumerate(layers):
        L[z].src, L[z].irow = a.ctypes.data, a.strides[0]
        L[z].width, L[z].height, L[z].offs_x, L[z].offs_y, L[z].alpha = w, h, ox, oy, al
    before = blank(oh, align(ow * ps + 16))
    assert form == "k_composite<%d>" % ps
    want = before.copy()
    orc.orc_composite(P(want), want.strides[0], ow, oh, ps, is_bgr, (ctypes.c_int * 3)(*bg), L, len(layers), revz)
    kept(oh, (want, before))
    if gpu is None:
        return
    d = dev(before)
    gpu.composite(d, ow, oh, ps, [(dev(a), w, h, ox, oy, al) for (a, w, h, ox, oy, al) in layers], bgcol=bg, is_bgr=is_bgr, revz=revz)
    same_whole(host(d), want, before, oh, "composite ps=%d bgr=%d revz=%d width %d" % (ps, is_bgr, revz, ow))


for _ps, _bgr, _revz in ((3, 0, 0), (4, 1, 1)):
    for _w in both(K_COMP):
        add("composite", "k_composite<%d>" % _ps, run_composite, _ps, _bgr ^ (_w & 1), _revz, _w)
FORMS["composite"] = {"k_composite<3>", "k_composite<4>"}


def run_transition(orc, gpu, tune, form, kind, ps, amt, w, n=1):
    h, S = SPANS[K_TRANS].rows, SPANS[K_TRANS].span
    rng = seeded("transition", kind, ps, amt, w, n)
    st = align(w * ps + 16)
    assert form == "k_transition<%d>" % ps
    if kind == 0 and w > 2 * S:
        xx = int(int(np.float32(w * ps) * np.float32(0.5)) * (np.float32(1.) - np.float32(amt)) + .5)             # the rectangle's inset in bytes, as the host code has it
        assert (w * ps - xx) // ps > S, "the rectangle's right edge at pixel %d is not beyond the first %d pixels of the row" % ((w * ps - xx) // ps, S)
    if kind == 1 and w > 2 * S:
        # the circle around (w / 2, h / 2) with radius amt * sqrt((w / 2)^2 + (h / 2)^2): where it leaves the middle row on the right
        edge = w / 2. + amt * ((w / 2.) ** 2 + (h / 2.) ** 2) ** .5
        assert S < edge < w, "the circle's right edge at pixel %d is not beyond the first %d pixels of the row" % (edge, S)
    if kind == 2 and w > 2 * S:
        # the cross's vertical bar spans |x - w / 2| < amt * w / 2; right of it the quadrants are shifted copies
        edge = w / 2. * (1. + amt)
        assert S < edge < w, "the right edge of the cross at pixel %d is not beyond the first %d pixels of the row" % (edge, S)
    s1, s2 = [src_frame(rng, w, h, ps, st) for _ in range(n)], [src_frame(rng, w, h, ps, st) for _ in range(n)]
    before = blank(h, st)
    wants = []
    for f in range(n):
        wt = before.copy()
        orc.orc_transition(kind, P(s1[f]), st, P(s2[f]), st, P(wt), st, w, h, ps, amt)
        wants.append(wt)
    wip = None
    if kind < 2:
        wip = s1[0].copy()
        orc.orc_transition(kind, P(wip), st, P(s2[0]), st, P(wip), st, w, h, ps, amt)
    kept(h, *[(wt, before) for wt in wants] + ([(wip, s1[0])] if wip is not None else []))
    if gpu is None:
        return
    what = "transition %d ps=%d amount=%s width %d" % (kind, ps, amt, w)
    if n > 1:
        d1, d2, dd = [dev(a) for a in s1], [dev(a) for a in s2], [dev(before) for _ in range(n)]
        gpu.fx_batch(ta.FX["transition"], [[t] for t in d1], [[t] for t in dd], w, h, ins1=[[t] for t in d2], ip=(kind, ps), dp=(amt,))
        for f in range(n):
            same_whole(host(dd[f]), wants[f], before, h, what + " fx_batch frame %d" % f)
        return
    d = dev(before)
    gpu.transition(kind, dev(s1[0]), dev(s2[0]), d, w, h, ps, amt)
    same_whole(host(d), wants[0], before, h, what)
    if wip is not None:
        d = dev(s1[0])
        gpu.transition(kind, d, dev(s2[0]), d, w, h, ps, amt)
        same_whole(host(d), wip, s1[0], h, what + " in place")


for _kind in (0, 1, 2):
    for _ps, _amt in ((3, 0.25), (4, 0.73)):
        for _w in both(K_TRANS, lo=2):
            add("transition", "k_transition<%d>" % _ps, run_transition, _kind, _ps, _amt, _w)
    add("transition", "k_transition<4>", run_transition, _kind, 4, 0.25, widths(K_TRANS, lo=2)[0][1], 3)
FORMS["transition"] = {"k_transition<3>", "k_transition<4>"}


def run_slide_over(orc, gpu, tune, form, ps, dirn, tv, mvl, mvu, w):
    h, S = H3, SPANS[K_COL].span
    rng = seeded("slide", ps, dirn, tv, mvl, mvu, w)
    st = align(w * ps + 16)
    assert form == "k_slide_over<%d>" % ps
    if dirn <= 2 and w > 2 * S:
        bound = int(np.float32(w) * (1. - tv / 255.)) if dirn == 1 else int(np.float32(w) * (tv / 255.))
        assert S < bound < w, "the dividing column %d is not in the second workgroup" % bound
    s1, s2 = src_frame(rng, w, h, ps, st), src_frame(rng, w, h, ps, st)
    before = blank(h, st)
    want = before.copy()
    orc.orc_slide_over(P(s1), st, P(s2), st, P(want), st, w, h, ps, tv, dirn, mvl, mvu)
    kept(h, (want, before))
    if gpu is None:
        return
    d = dev(before)
    gpu.slide_over(dev(s1), dev(s2), d, w, h, ps, tv, dirn, mvl, mvu)
    same_whole(host(d), want, before, h, "slide over ps=%d dir=%d amount=%d lower=%d upper=%d width %d" % (ps, dirn, tv, mvl, mvu, w))


for _ps, _dirn, _tv, _mvl, _mvu in ((3, 1, 77, 1, 0), (4, 2, 200, 0, 1), (4, 1, 60, 1, 1), (3, 2, 170, 0, 0), (4, 3, 128, 1, 0), (3, 4, 90, 0, 1)):
    for _w in both(K_COL):
        add("slide_over", "k_slide_over<%d>" % _ps, run_slide_over, _ps, _dirn, _tv, _mvl, _mvu, _w)
FORMS["slide_over"] = {"k_slide_over<3>", "k_slide_over<4>"}


def run_triple_split(orc, gpu, tune, form, is_bgr, start, sym, end, vert, bw, w):
    h, S = H3, SPANS[K_COL].span
    rng = seeded("split", is_bgr, start, sym, end, vert, bw, w)
    bc = np.array([13, 250, 77], np.int32)
    st = align(w * 3 + 16)
    assert form == "k_triple_split"
    if not vert and w > 2 * S:
        xs, xe = (start / 2., 1. - start / 2.) if sym else (start, end)
        cols = [3 * w * v / 3. for v in (xs - bw, xs + bw, xe - bw, xe + bw)]
        assert sum(S < c < w for c in cols) >= 2, "no split column in the second workgroup: %s" % cols
    s1, s2 = src_frame(rng, w, h, 3, st), src_frame(rng, w, h, 3, st)
    before = blank(h, st)
    want, wip = before.copy(), s1.copy()
    orc.orc_triple_split(P(s1), st, P(s2), st, P(want), st, w, h, is_bgr, start, sym, end, vert, bw, bc.ctypes.data)
    orc.orc_triple_split(P(wip), st, P(s2), st, P(wip), st, w, h, is_bgr, start, sym, end, vert, bw, bc.ctypes.data)
    kept(h, (want, before), (wip, s1))
    if gpu is None:
        return
    what = "triple split %r width %d" % ((start, sym, end, vert, bw), w)
    d = dev(before)
    gpu.triple_split(dev(s1), dev(s2), d, w, h, is_bgr, start, sym, end, vert, bw, bc)
    same_whole(host(d), want, before, h, what)
    d = dev(s1)
    gpu.triple_split(d, dev(s2), d, w, h, is_bgr, start, sym, end, vert, bw, bc)
    same_whole(host(d), wip, s1, h, what + " in place")


for _bgr, _prm in ((0, (0.55, 0, 0.8, 0, 0.02)), (1, (0.666667, 1, 0.333333, 0, 0.04)), (0, (0.4, 1, 0.0, 1, 0.07))):
    for _w in both(K_COL):
        add("triple_split", "k_triple_split", run_triple_split, _bgr, *(_prm + (_w,)))
FORMS["triple_split"] = {"k_triple_split"}


def run_dissolve(orc, gpu, tune, form, ps, amt, w):
    h = H3
    rng = seeded("dissolve", ps, amt, w)
    seed = 0xC0FFEE + w
    mask = np.zeros(w * h, np.float32)
    orc.orc_dissolve_mask(seed, w, h, mask.ctypes.data)
    st = align(w * ps + 16)
    assert form == "k_dissolve<%d>" % ps
    s1, s2 = src_frame(rng, w, h, ps, st), src_frame(rng, w, h, ps, st)
    before = blank(h, st)
    want, wip = before.copy(), s1.copy()
    orc.orc_dissolve(P(s1), st, P(s2), st, P(want), st, w, h, ps, mask.ctypes.data, amt)
    orc.orc_dissolve(P(wip), st, P(s2), st, P(wip), st, w, h, ps, mask.ctypes.data, amt)
    kept(h, (want, before), (wip, s1))
    if gpu is None:
        return
    import torch
    gm = gpu.dissolve_mask(seed, w, h)
    assert (gm == mask).all()
    dm = torch.from_numpy(gm).cuda()
    d = dev(before)
    gpu.dissolve(dev(s1), dev(s2), d, w, h, ps, dm, amt)
    same_whole(host(d), want, before, h, "dissolve ps=%d amount=%s width %d" % (ps, amt, w))
    d = dev(s1)
    gpu.dissolve(d, dev(s2), d, w, h, ps, dm, amt)
    same_whole(host(d), wip, s1, h, "dissolve ps=%d amount=%s width %d in place" % (ps, amt, w))


for _ps, _amt in ((3, 0.37), (4, 0.5)):
    for _w in both(K_COL):
        add("dissolve", "k_dissolve<%d>" % _ps, run_dissolve, _ps, _amt, _w)
FORMS["dissolve"] = {"k_dissolve<3>", "k_dissolve<4>"}


# ---- runtime.hip
K_FILL = ("runtime.hip", "cdiv(nbytes,kBlock)")


def run_fill_pattern(orc, gpu, tune, form, plen, n):
    """lgpu_fill_pattern against a numpy fill: n repeats of a pattern of plen bytes per row (the table counts bytes: n * plen of them)"""
    rows = H3
    rng = seeded("fill", plen, n)
    before = rng.integers(0, 256, (rows + GUARD, n * plen + 9), dtype=np.uint8)
    pat = rng.integers(0, 256, plen, dtype=np.uint8)
    assert form == "k_fill_pattern"
    want = before.copy()
    want[:rows, :n * plen] = np.tile(pat, n)
    kept(rows, (want, before))
    if gpu is None:
        return
    d = dev(before)
    gpu.lib.call("lgpu_fill_pattern", d.data_ptr(), before.strides[0], pat.ctypes.data, plen, n, rows, None)
    same_whole(host(d), want, before, rows, "fill_pattern plen=%d x %d" % (plen, n))


for _plen in (1, 3, 4, 8):
    for _b in both(K_FILL, g=_plen, lo=_plen):
        add("fill_pattern", "k_fill_pattern", run_fill_pattern, _plen, _b // _plen)
FORMS["fill_pattern"] = {"k_fill_pattern"}


# ---- palette.hip: RGB -> YUV, YUV -> RGB (the runners of tests/test_tall_frames.py: every plane on a pitch that is a multiple of 16, so the width and the pixel sizes
# alone decide the form -- all address bits are 0 in the restated rule)
K_K4 = ("palette.hip", "cdiv(npairs,kBlock)")
K4S = {n: ("palette.hip", "cells(width>>2)/512:k_rgb_to_yuv%s_s" % n) for n in ("420", "422", "444")}


def run_rgb_to_yuv(orc, gpu, tune, form, order, ia, fmt, w, h, n=1):
    ips, oa = 4 if (order == 2 or ia) else 3, 1 if (fmt <= 1 and order == 0) else 0
    assert ta.rule_rgb_to_yuv(fmt, ips, order, oa, w, 0, 0, 0, 0) == form
    tt.run_rgb_to_yuv(orc, gpu, order, ia, w, fmt, h, n)


def k4_heights(fmt):
    """4:2:0 walks row pairs (the cell form: row 0 alone, pairs, the trailing row): 4 and 6 rows; every other target is pointwise"""
    return (4, 6) if fmt == 4 else (H3,)


for _fmt in range(6):
    _g = 1 if _fmt < 2 else 2
    # the generic kernel: 3-byte pixels (every subsampled target), ARGB, and widths that are no multiple of 4
    for _order, _ia in ((0, 0), (1, 0), (2, 1)) if _fmt < 4 else ((0, 0), (1, 0)):
        for _w in both(K_K4, g=_g, lo=_g):
            _ips = 4 if (_order == 2 or _ia) else 3
            _form = ta.rule_rgb_to_yuv(_fmt, _ips, _order, 1 if (_fmt <= 1 and _order == 0) else 0, _w, 0, 0, 0, 0)
            if _form == "k_rgb_to_yuv":
                for _h in k4_heights(_fmt):
                    add("rgb_to_yuv", _form, run_rgb_to_yuv, _order, _ia, _fmt, _w, _h)
    _name = "444" if _fmt < 2 else "420" if _fmt == 4 else "422"
    for _order, _ia in ((0, 1), (1, 1)) + (((0, 0), (1, 0)) if _fmt < 2 else ()):
        for _w in both(K4S[_name]):
            for _h in k4_heights(_fmt):
                add("rgb_to_yuv", "k_rgb_to_yuv%s_s" % _name, run_rgb_to_yuv, _order, _ia, _fmt, _w, _h)
for _fmt, _w in ((0, widths(K4S["444"])[0][2]), (2, widths(K4S["422"])[0][2]), (4, widths(K4S["420"])[0][2]), (3, widths(K_K4, g=2, lo=2)[0][1])):
    add("rgb_to_yuv", ta.rule_rgb_to_yuv(_fmt, 4, 0, 1 if _fmt <= 1 else 0, _w, 0, 0, 0, 0), run_rgb_to_yuv, 0, 1, _fmt, _w, 4 if _fmt == 4 else 3, 3)
FORMS["rgb_to_yuv"] = {"k_rgb_to_yuv", "k_rgb_to_yuv420_s", "k_rgb_to_yuv422_s", "k_rgb_to_yuv444_s"}

K_K3 = ("palette.hip", "cdiv(((width+1)>>1),kBlock)")
K3S = {n: ("palette.hip", "cells(width>>2)/512:%s" % n) for n in ("k_uyvy_to_rgb_s", "k_yuv444_to_rgb_s")}


def run_yuv_to_rgb(orc, gpu, tune, form, fmt, ia, order, oa, w):
    ops = 4 if (order == 2 or oa) else 3
    assert ta.rule_yuv_to_rgb(fmt, ia, ops, w, 0, 0, 0) == form
    tt.run_yuv_to_rgb(orc, gpu, fmt, ia, order, oa, w, H3)


for _fmt, _ia, _order, _oa in ((0, 0, 0, 0), (0, 1, 2, 1), (1, 0, 0, 1), (1, 1, 1, 1), (2, 0, 0, 0), (2, 0, 2, 1), (3, 0, 1, 0), (3, 0, 0, 1)):
    _ops = 4 if (_order == 2 or _oa) else 3
    _g = 1 if _fmt < 2 else 2
    for _w in both(K_K3, g=_g, lo=_g):
        if ta.rule_yuv_to_rgb(_fmt, _ia, _ops, _w, 0, 0, 0) == "k_yuv_to_rgb":
            add("yuv_to_rgb", "k_yuv_to_rgb", run_yuv_to_rgb, _fmt, _ia, _order, _oa, _w)
    _cell = "k_uyvy_to_rgb_s" if (_fmt >= 2 and _ops == 4) else "k_yuv444_to_rgb_s" if _fmt < 2 else None
    if _cell:
        for _w in both(K3S[_cell]):
            add("yuv_to_rgb", _cell, run_yuv_to_rgb, _fmt, _ia, _order, _oa, _w)


def run_yuv_to_rgb_batch(orc, gpu, tune, form, fmt, ia, order, oa, w, n):
    """lgpu_yuv_to_rgb_batch: the frame is blockIdx.z of the generic kernel and of the cell kernels"""
    h, ops = H3, 4 if (order == 2 or oa) else 3
    assert ta.rule_yuv_to_rgb(fmt, ia, ops, w, 0, 0, 0) == form
    rng = seeded("yuv_to_rgb_batch", fmt, ia, order, oa, w, n)
    which = (1 if oa else 0) | (2 if (fmt == 0 and ia) else 0)
    dims = [(w * (4 if ia else 3), h)] if fmt == 0 else [(w, h)] * (4 if ia else 3) if fmt == 1 else [(w * 2, h)]
    planes = [[rng.integers(0, 256, (b + GUARD, align(a)), dtype=np.uint8) for (a, b) in dims] for _ in range(n)]
    before = blank(h, align(w * ops + 16))
    wants = []
    for f in range(n):
        wt = before.copy()
        sp, ss = po.planes_args(planes[f])
        assert orc.orc_yuv_to_rgb(ctypes.addressof(sp), ctypes.addressof(ss), w, h, fmt, ia, P(wt), wt.strides[0], order, oa, which) == 0
        wants.append(wt)
    kept(h, *[(wt, before) for wt in wants])
    if gpu is None:
        return
    dd = [dev(before) for _ in range(n)]
    gpu.yuv_to_rgb_batch([[dev(a) for a in fr] for fr in planes], dd, w, h, fmt, ia, order, oa, which)
    for f in range(n):
        same_whole(host(dd[f]), wants[f], before, h, "yuv_to_rgb batch fmt=%d ia=%d order=%d oa=%d width %d frame %d" % (fmt, ia, order, oa, w, f))


add("yuv_to_rgb", "k_yuv_to_rgb", run_yuv_to_rgb_batch, 2, 0, 0, 0, widths(K_K3, g=2, lo=2)[0][1], 3)
add("yuv_to_rgb", "k_uyvy_to_rgb_s", run_yuv_to_rgb_batch, 3, 0, 0, 1, widths(K3S["k_uyvy_to_rgb_s"])[0][2], 3)
add("yuv_to_rgb", "k_yuv444_to_rgb_s", run_yuv_to_rgb_batch, 1, 1, 1, 1, widths(K3S["k_yuv444_to_rgb_s"])[0][2], 3)
FORMS["yuv_to_rgb"] = {"k_yuv_to_rgb", "k_uyvy_to_rgb_s", "k_yuv444_to_rgb_s"}


# ---- palette.hip: lgpu_yuv_repack and the 4:1:1 conversions
K_RPK, K_CUP, K_411 = ("palette.hip", "cdiv(((span+1)>>1),kBlock)"), ("palette.hip", "cdiv((width>>1),kBlock)"), ("palette.hip", "cdiv((width>>2),kBlock)")
RPK_S = {n: ("palette.hip", "cells(width>>%d)/512:%s" % (s, n)) for n, s in (("k_420_to_packed_s", 3), ("k_combine_s", 2), ("k_split_s", 2), ("k_swab_s", 3), ("k_pk_to_s", 3),
                                                                            ("k_888_to_s", 2), ("k_420_to_422p_s", 3))}
RPK_H = 4           # even, two row pairs: every 4:2:0 side of the pairs below


def repack_form(ip, op, w, pad):
    ir = [nb + pad for (nb, _) in po.YUV_PLANE_DIMS[ip](w, RPK_H)] + [0] * 4
    orw = [nb + pad for (nb, _) in po.YUV_PLANE_DIMS[op](w, RPK_H)] + [0] * 4
    return ta.rule_repack(ip, op, w, [0] * 4, ir, [0] * 4, orw)


def run_repack(orc, gpu, tune, form, ip, op, pad, w):
    assert repack_form(ip, op, w, pad) == form
    tt.run_repack(orc, gpu, ip, op, w, RPK_H, pad, (ip + op + w) & 1, 0, "repack")


# one pair per `_s` kernel and kind, at the kernel's own widths; then every pair that has a kernel of its own at the widths of k_yuv_repack, where the restated rule
# says which kernel takes it
for _cell, _pairs in (("k_420_to_packed_s", ((512, 564), (522, 565))), ("k_combine_s", ((544, 588), (545, 589))), ("k_split_s", ((588, 544),)), ("k_swab_s", ((564, 565),)),
                      ("k_pk_to_s", ((564, 512), (565, 544), (564, 589), (565, 588))), ("k_888_to_s", ((588, 512), (589, 522), (588, 564), (589, 565))), ("k_420_to_422p_s", ((512, 522),))):
    for _ip, _op in _pairs:
        _padok = [p for p in po.YUV_REPACK_PAIRS if p[:2] == (_ip, _op)][0][2]
        for _w in both(RPK_S[_cell]):
            add("repack", _cell, run_repack, _ip, _op, 32 if _padok else 0, _w)
for _ip, _op, _padok in tt.RPK_PAIRS:
    for _w in both(K_RPK, g=2, lo=2):
        _form = repack_form(_ip, _op, _w, 24 if _padok else 0)
        if _form == "k_yuv_repack":
            add("repack", _form, run_repack, _ip, _op, 24 if _padok else 0, _w)
FORMS["repack"] = set(RPK_S) | {"k_yuv_repack"}


def run_chroma_up(orc, gpu, tune, form, ip, op, sampling, w):
    assert form == "k_chroma_up_packed"
    tt.run_repack(orc, gpu, ip, op, w, SPANS[K_CUP].rows, 24, w & 1 ^ (w >> 1) & 1, sampling, "chroma up")


for _ip, _op in po.CHROMA_UP_PAIRS:
    for _w in both(K_CUP, g=2, lo=2):
        add("chroma_up", "k_chroma_up_packed", run_chroma_up, _ip, _op, (_w >> 1) & 1, _w)
FORMS["chroma_up"] = {"k_chroma_up_packed"}


def run_rgb_to_yuv411(orc, gpu, tune, form, order, ia, w):
    assert form == "k_rgb_to_yuv411"
    tt.run_rgb_to_yuv411(orc, gpu, order, ia, w, H3)


def run_r411(orc, gpu, tune, form, ip, op, padok, w):
    assert ta.rule_repack(ip, op, w, [0] * 4, [0] * 4, [0] * 4, [0] * 4) == form
    h, pad, unc = SPANS[K_411].rows, (24 if padok else 0), (ip + op + (w >> 2)) & 1
    rng = seeded("r411", ip, op, w)
    src = tt.planes_of(ip, w, h, pad, rng)
    before = tt.planes_of(op, w, h, 0)
    want = [b.copy() for b in before]
    sp, ss = po.planes_args(src)
    wp, ws = po.planes_args(want)
    assert orc.orc_yuv_repack(ip, op, ctypes.addressof(sp), ctypes.addressof(ss), ctypes.addressof(wp), ctypes.addressof(ws), w, h, unc, 0) == 0
    for i, (nb, rows) in enumerate(po.YUV_PLANE_DIMS[op](w, h)):
        kept(rows, (want[i], before[i]))
    if gpu is None:
        return
    dst = [dev(b) for b in before]
    gpu.yuv_repack(ip, op, [dev(a) for a in src], dst, w, h, unc)
    for i, (nb, rows) in enumerate(po.YUV_PLANE_DIMS[op](w, h)):
        same_whole(host(dst[i]), want[i], before[i], rows, "411 repack %d->%d width %d unclamped=%d pad=%d plane %d" % (ip, op, w, unc, pad, i))


# the reference cuts a frame's right edge to whole macropixels: every width from 4 (the minimum the fuzzer draws), a multiple of 4 or not, for RGB -> 4:1:1
for _order, _ia in ((0, 0), (1, 1), (2, 1)):
    for _w in both(K_411, lo=4):
        add("yuv411", "k_rgb_to_yuv411", run_rgb_to_yuv411, _order, _ia, _w)
for _ip, _op, _padok in po.YUV411_REPACK_PAIRS:
    for _w in both(K_411, g=4, lo=4):
        add("yuv411", "k_yuv411_repack", run_r411, _ip, _op, _padok, _w)


def run_yuv411_to_rgb(orc, gpu, tune, form, order, oa, uncl, w, n=1):
    """macropixels of four pixels run on from row to row: the second workgroup begins in the middle of a row"""
    assert form == "k_yuv411_to_rgb"
    wm, h = w >> 2, H3
    ps = 4 if (order == 2 or oa) else 3
    rng = seeded("yuv411_to_rgb", order, oa, uncl, w, n)
    srcs = [rng.integers(0, 256, (h + GUARD, wm * 6), dtype=np.uint8) for _ in range(n)]
    before = blank(h, wm * 4 * ps + 32)
    wants = []
    for s in srcs:
        wt = before.copy()
        assert orc.orc_yuv411_to_rgb(P(s), wm, h, P(wt), wt.strides[0], order, oa, uncl) == 0
        wants.append(wt)
    kept(h, *[(wt, before) for wt in wants])
    if gpu is None:
        return
    d_s, d_o = [dev(s) for s in srcs], [dev(before) for _ in range(n)]
    if n > 1:
        gpu.fx_batch(ta.FX["yuv411_to_rgb"], [[t] for t in d_s], [[t] for t in d_o], wm, h, ip=(order, oa, uncl))
    else:
        gpu.yuv411_to_rgb(d_s[0], d_o[0], wm, h, out_order=order, out_alpha=oa, unclamped=uncl)
    for f in range(n):
        same_whole(host(d_o[f]), wants[f], before, h, "yuv411_to_rgb order=%d alpha=%d unclamped=%d width %d frame %d" % (order, oa, uncl, w, f))


K_411R = ("palette.hip", "cdiv(ncells,kBlock)")
for _order, _oa, _uncl in ((0, 0, 0), (1, 1, 1), (2, 1, 0)):
    for _w in both(K_411R, g=4, lo=4):
        add("yuv411", "k_yuv411_to_rgb", run_yuv411_to_rgb, _order, _oa, _uncl, _w)
add("yuv411", "k_yuv411_to_rgb", run_yuv411_to_rgb, 0, 1, 0, widths(K_411R, g=4, lo=4)[0][1], 3)
FORMS["yuv411"] = {"k_rgb_to_yuv411", "k_yuv411_repack", "k_yuv411_to_rgb"}


K_CLAMP = ("palette.hip", "cdiv(((n0+15)/16),kBlock)")


def run_clamp_switch(orc, gpu, tune, form, to_unclamped, w):
    """one YUVA8888 plane of 3 rows whose pitch is the row: the kernel walks the plane's bytes as one stream, so the table's bytes are the whole plane's"""
    assert form == "k_clamp_switch"
    h = H3
    rng = seeded("clamp", to_unclamped, w)
    plane = rng.integers(0, 256, (h + GUARD, w * 4), dtype=np.uint8)
    want = [plane.copy()]
    wp, ws = po.planes_args(want)
    assert orc.orc_switch_yuv_clamping(ctypes.addressof(wp), ctypes.addressof(ws), 589, h, to_unclamped) == 0
    kept(h, (want[0], plane))
    if gpu is None:
        return
    d = dev(plane)
    gpu.yuv_switch_clamping([d], 589, h, to_unclamped)
    same_whole(host(d), want[0], plane, h, "switch clamping to_unclamped=%d width %d" % (to_unclamped, w))


for _b in both(K_CLAMP, g=12, lo=12):                  # 3 rows of 4-byte pixels: a plane of 12 bytes per pixel of width
    add("clamp_switch", "k_clamp_switch", run_clamp_switch, (_b // 12) & 1, _b // 12)
FORMS["clamp_switch"] = {"k_clamp_switch"}


# ---- yuv.hip
K_K2, K_K2S = ("yuv.hip", "cdiv((width>>1),kBlock)"), ("yuv.hip", "cells(ncg)/s_block:k_yuv420p_to_rgb_s")


def run_yuv420p(orc, gpu, tune, form, opsize, q, use_lut, order, is422, fix, nc, w, h, n=1):
    """lgpu_yuv420p_to_rgb; nc: the chroma columns per lane of the cell form (lgpu_yuv420_tuning), 0 switches that form off"""
    rng = seeded("k2", opsize, q, use_lut, order, is422, fix, nc, w, h, n)
    lut = tt.l2s_lut(orc) if use_lut else None
    ch = h if is422 else (h + 1) // 2
    ys, cs = align(w, 16) + 16, align(w >> 1, 16)
    fr = [(rng.integers(0, 256, (h + GUARD, ys), dtype=np.uint8), rng.integers(0, 256, (ch, cs), dtype=np.uint8), rng.integers(0, 256, (ch, cs), dtype=np.uint8)) for _ in range(n)]
    Y, U, V = fr[0]
    before = blank(h, align(w * opsize + 16))
    ops = 4 if order == 2 else opsize
    rule = ta.rule_yuv420p(ops, 0, q == 1, ys, before.strides[0], nc) if nc else "k_yuv420p_to_rgb"
    assert rule == form
    strides = (ctypes.c_int * 3)(ys, cs, cs)
    which = int(rng.integers(0, 4))
    wants = []
    for (y_, u_, v_) in fr:
        wt = before.copy()
        orc.orc_yuv420p_to_rgb(P(y_), P(u_), P(v_), strides, u_.size, v_.size, P(wt), wt.strides[0], w, h, opsize, order, is422, which, q, P(lut), fix)
        wants.append(wt)
    want = wants[0]
    kept(h, *[(wt, before) for wt in wants])
    if gpu is None:
        return
    L = gpu.lib.load()                              # (the library handle: the tuning call has no wrapper)
    d = dev(before)
    flags = gpu.lib.YUV_FIX_EDGES if fix else 0
    L.lgpu_yuv420_tuning(nc, -1, -1)
    try:
        if n > 1:                                   # lgpu_yuv420p_to_rgb_batch: the frame is blockIdx.y (cell form) / blockIdx.z
            dd = [dev(before) for _ in range(n)]
            gpu.yuv420p_to_rgb_batch([(dev(y_), dev(u_), dev(v_), dd[f]) for f, (y_, u_, v_) in enumerate(fr)], w, h, opsize=opsize, out_order=order, is_422=is422, which_tables=which,
                                     pb_quality=q, lut=lut, flags=flags)
            for f in range(n):
                same_whole(host(dd[f]), wants[f], before, h, "yuv420p batch nc=%d %dx%d frame %d" % (nc, w, h, f))
            return
        gpu.yuv420p_to_rgb(dev(Y), dev(U), dev(V), d, w, h, opsize=opsize, out_order=order, is_422=is422, which_tables=which, pb_quality=q, lut=lut,
                           flags=flags, u_size=U.size, v_size=V.size)
    finally:
        L.lgpu_yuv420_tuning(2, 512, 8)
    same_whole(host(d), want, before, h, "yuv42%dp opsize=%d quality=%d lut=%d order=%d fix=%d nc=%d %dx%d" % (2 if is422 else 0, opsize, q, use_lut, order, fix, nc, w, h))


for _is422 in (0, 1):
    for _h in ((6, 5) if not _is422 else (3,)):
        # the one-column kernels: 3-byte output, the LOW quality setting, and the cell form switched off
        for _opsize, _q, _lut, _order, _nc in ((3, 2, 0, 0, 2), (4, 1, 1, 1, 2), (4, 2, 0, 2, 0)):
            for _w in both(K_K2, g=2, lo=2):
                add("yuv420p", "k_yuv420p_to_rgb", run_yuv420p, _opsize, _q, _lut, _order, _is422, (_w >> 1) & 1 if not _is422 else 0, _nc, _w, _h)
        # the cell form at every NC: a cell is 2 NC pixels wide, 512 lanes a workgroup
        for _nc in (1, 2, 4):
            _u = 2 * _nc
            for _w in both(K_K2S, g=2, lo=2, unit=_u):
                add("yuv420p", "k_yuv420p_to_rgb_s", run_yuv420p, 4, 2 + (_w >> 1 & 1), _nc & 1, (_w >> 2) % 3, _is422, (_w >> 1) & 1 if not _is422 else 0, _nc, _w, _h)
add("yuv420p", "k_yuv420p_to_rgb_s", run_yuv420p, 4, 2, 0, 0, 0, 1, 2, widths(K_K2S, g=2, lo=2)[0][2], 6, 3)
add("yuv420p", "k_yuv420p_to_rgb", run_yuv420p, 3, 2, 1, 1, 1, 0, 2, widths(K_K2, g=2, lo=2)[0][1], 3, 3)
FORMS["yuv420p"] = {"k_yuv420p_to_rgb", "k_yuv420p_to_rgb_s"}


# ---- stencil.hip
K_SOFTC, K_EPAINT4 = ("stencil.hip", "cdiv(cp.w,256u)"), ("stencil.hip", "cells(quads)/kBlock")
K_SOFTS, K_TILE, K_EPAINT, K_EMAP4 = ("stencil.hip", "cdiv((width>>2),62u)"), ("stencil.hip", "cdiv(width,kStW)"), ("stencil.hip", "cdiv(width,kBlock)"), ("stencil.hip", "cdiv(width,kEmW)")
K_BZV, K_BZB, K_DEINT = ("stencil.hip", "cdiv(vw,kBlock)"), ("stencil.hip", "cdiv(bw,kBlock)"), ("stencil.hip", "cdiv(a.ntrip,kBlock)")
K_RGBDS, K_RGBD, K_RGBD4 = ("stencil.hip", "cdiv(wb,kBlock)"), ("stencil.hip", "cdiv(span,kBlock)"), ("stencil.hip", "cdiv(((orow+11)/12),kBlock)")


def run_softlight(orc, gpu, tune, form, palette, pf, w, n=1):
    h = SPANS[K_SOFTS].rows
    rng = seeded("softlight", palette, pf, w, n)
    cw, chh = (w >> 1 if palette in (512, 513, 522) else w), (h >> 1 if palette in (512, 513) else h)
    dims = [(w, h), (cw, chh), (cw, chh)] + ([(w, h)] if palette == 545 else [])
    lp = align(w + 4, 4) if pf == "v" else (w + 1) | 1
    pit = lambda k, a: lp if k == 0 else a + 3
    assert ta.rule_softlight(w, lp) == form
    src = [[rng.integers(0, 256, (b + GUARD, pit(k, a)), dtype=np.uint8) for k, (a, b) in enumerate(dims)] for _ in range(n)]
    before = [np.full((b + GUARD, pit(k, a)), FILL, np.uint8) for k, (a, b) in enumerate(dims)]
    wants = []
    for f in range(n):
        wt = [b.copy() for b in before]
        orc.orc_softlight_y(P(src[f][0]), src[f][0].strides[0], P(wt[0]), wt[0].strides[0], w, h, 0)
        for k, (a, b) in enumerate(dims[1:], 1):
            wt[k][:b, :a] = src[f][k][:b, :a]
        wants.append(wt)
    for wt in wants:
        for k, (a, b) in enumerate(dims):
            kept(b, (wt[k], before[k]))
    if gpu is None:
        return
    d_s, d_o = [[dev(a) for a in fr] for fr in src], [[dev(b) for b in before] for _ in range(n)]
    if n > 1:
        gpu.fx_batch(ta.FX["softlight"], d_s, d_o, w, h, palette=palette, ip=(0,))
    else:
        gpu.softlight(d_s[0], d_o[0], w, h, palette, 0)
    for f in range(n):
        for k, (a, b) in enumerate(dims):
            same_whole(host(d_o[f][k]), wants[f][k], before[k], b, "softlight %d %s width %d frame %d plane %d" % (palette, pf, w, f, k))


# softlight needs 3 x 3 samples, and the fuzzer draws even widths from 4: the strip form takes multiples of 4 from 8, the tile kernel everything else
for _pal in (544, 545, 522, 512):
    _g = 2 if _pal in (522, 512) else 1
    # the copied planes are as wide as the luma plane (4:4:4) or half as wide: their tiles of 256 bytes end at other widths than the strips
    _copy = [_w * (2 if _pal in (522, 512) else 1) for _w in widths(K_SOFTC, g=4, lo=8)[0]]
    for _w in sorted(set(both(K_SOFTS, g=4, lo=8) + _copy)):
        add("softlight", "k_softlight_s", run_softlight, _pal, "v", _w)
    for _w in both(K_TILE, g=_g, lo=4):
        add("softlight", ta.rule_softlight(_w, (_w + 1) | 1), run_softlight, _pal, "b", _w)
        if _w & 3:
            add("softlight", "k_softlight", run_softlight, _pal, "v", _w)
add("softlight", "k_softlight_s", run_softlight, 545, "v", widths(K_SOFTS, g=4, lo=8)[0][1], 3)
add("softlight", "k_softlight", run_softlight, 512, "b", widths(K_TILE, g=2, lo=4)[0][1], 3)
FORMS["softlight"] = {"k_softlight_s", "k_softlight"}


def run_edge(orc, gpu, tune, form, pal, mode, pf, w):
    ps, h = 3 if pal <= 2 else 4, SPANS[K_EMAP4].rows
    rng = seeded("edge", pal, mode, pf, w)
    st = pitch(w, ps, pf)
    assert ta.rule_edge(ps, w, st) == form
    s = src_frame(rng, w, h, ps, st)
    yy, xx = np.mgrid[0:h, 0:w]                      # smooth structure under the noise so that the histogram is not flat
    for c in range(ps):
        s[:h, c:w * ps:ps] = ((s[:h, c:w * ps:ps] >> 3) + (96 * ((xx // 9 + yy // 2 + c) % 2)).astype(np.uint8) + 40).astype(np.uint8)
    d0 = rng.integers(0, 256, s.shape, dtype=np.uint8)
    want, wip = d0.copy(), s.copy()
    m16 = np.zeros(w * h, np.int16)
    orc.orc_edge(P(s), st, P(want), st, w, h, pal, mode, P(m16), 0)
    orc.orc_edge(P(wip), st, P(wip), st, w, h, pal, mode, P(m16), 1)
    kept(h, (want, d0), (wip, s))
    if gpu is None:
        return
    d = dev(d0)
    gpu.edge(dev(s), d, w, h, pal, mode)
    same_whole(host(d), want, d0, h, "edge pal=%d mode=%d %s width %d" % (pal, mode, pf, w))
    d = dev(s)
    gpu.edge(d, d, w, h, pal, mode)
    same_whole(host(d), wip, s, h, "edge pal=%d mode=%d %s width %d in place" % (pal, mode, pf, w))


# the fuzzer draws edge frames from 4 x 4; the quad form takes 4-byte pixels at multiples of 4 from 8 on 16-byte rows
EDGE_W = sorted(set(both(K_TILE, lo=4) + both(K_EPAINT, lo=4)))
for _pal, _mode in ((3, 2), (5, 0)):
    for _w in sorted(set(both(K_EMAP4, g=4, lo=8) + both(K_EPAINT4, g=4, lo=8))):
        add("edge", "k_edge_map4 + k_edge_paint4", run_edge, _pal, _mode, "v", _w)
for _pal, _mode, _pf in ((1, 0, "v"), (2, 2, "b"), (4, 1, "b"), (3, 0, "v")):
    for _w in EDGE_W:
        _form = ta.rule_edge(3 if _pal <= 2 else 4, _w, pitch(_w, 3 if _pal <= 2 else 4, _pf))
        if "map4" not in _form:
            add("edge", _form, run_edge, _pal, _mode, _pf, _w)
FORMS["edge"] = {"k_edge_map4 + k_edge_paint4", "k_edge_map<4> + k_edge_paint<4> dword", "k_edge_map<3> + k_edge_paint<3>"}


def run_deinterlace(orc, gpu, tune, form, pal, inplace, w):
    ps, h = 3 if pal in (1, 2, 588) else 4, SPANS[K_DEINT].rows
    st = align((w + 2) // 3 * 3 * ps, 32)            # the reference reads a partial last triple whole: the row has to hold it
    assert ta.rule_deinterlace(pal, w, inplace, st) == form
    rng = seeded("deinterlace", pal, w, inplace)
    s1 = src_frame(rng, w, h, ps, st)
    s1[1:h:2] = (s1[1:h:2] >> 2) + 160              # smooth vertical structure with comb rows so that both branches of the decision occur
    s1[0:h:2] = (s1[0:h:2] >> 2) + (rng.integers(0, 2, (s1[0:h:2].shape[0], 1), dtype=np.uint8) * 120)
    before = s1 if inplace else blank(h, st)
    want = before.copy()
    src = want if inplace else s1
    assert orc.orc_deinterlace(P(src), st, P(want), st, w, h, pal) == 0
    kept(h, (want, before))
    if gpu is None:
        return
    if inplace:
        d = dev(s1)
        gpu.deinterlace(d, d, w, h, pal)
    else:
        d = dev(before)
        gpu.deinterlace(dev(s1), d, w, h, pal)
    same_whole(host(d), want, before, h, "deinterlace pal=%d width %d inplace=%d" % (pal, w, inplace))


for _pal in (1, 588, 3, 589, 5, 564):
    for _inplace in ((1,) if _pal == 5 else (0, 1)):
        for _w in both(K_DEINT):
            add("deinterlace", ta.rule_deinterlace(_pal, _w, _inplace, 0), run_deinterlace, _pal, _inplace, _w)
FORMS["deinterlace"] = {"k_deinterlace dword", "k_deinterlace bytes"}


def run_rgbdelay(orc, gpu, tune, form, pal, inplace, w):
    """six frames through one ring whose parameters change after every second frame (the sequence of tests/test_tall_frames.py)"""
    assert ("k_rgbdelay4" if (3 * w) % 4 == 0 else "k_rgbdelay") == form           # rows of the runner are 32-byte multiples: the width decides
    tt.run_rgbdelay(orc, gpu, pal, w, inplace, H3)


for _pal, _inplace in ((1, 0), (2, 1), (588, 0)):
    # (k_rgbd_snapshot copies the 3 * width bytes of a row, a byte per lane)
    for _w in sorted(set(both(K_RGBD) + both(K_RGBD4, g=4, lo=4) + [b // 3 for b in both(K_RGBDS, g=3, lo=3)])):
        add("rgbdelay", "k_rgbdelay4" if _w % 4 == 0 else "k_rgbdelay", run_rgbdelay, _pal, _inplace, _w)
FORMS["rgbdelay"] = {"k_rgbdelay4", "k_rgbdelay"}


def run_blurzoom(orc, gpu, tune, form, pal, mode, pattern, w):
    assert form == "k_bz"
    h = SPANS[K_BZV].rows
    rng = seeded("blurzoom", pal, mode, pattern, w)
    seq = []
    for f in range(4):
        a = src_frame(rng, w, h, 4, w * 4 if mode in (1, 2) else align(w * 4 + 16))
        a[:h, :w * 4] = (a[:h, :w * 4] >> 4) + 40
        x0 = (8 + 37 * f) % max(1, w - 20)
        a[1 + (f & 1):4, x0 * 4:(x0 + 16) * 4] = 250             # a bright block that moves: the background subtraction fires on either side of the workgroup boundary
        a[2:5, max(0, w - 12 - 5 * f) * 4:w * 4] = 240
        seq.append(a)
    z = orc.orc_blurzoom_new(w, h, pal)
    wants = []
    for a in seq:
        want = np.full_like(a, FILL)
        assert orc.orc_blurzoom_process(z, P(a), a.strides[0], P(want), want.strides[0], mode, pattern) == 0
        wants.append(want)
    orc.orc_blurzoom_free(z)
    kept(h, *[(wt, np.full_like(wt, FILL)) for wt in wants])
    if gpu is None:
        return
    g = gpu.Blurzoom(w, h, pal)
    try:
        for f, a in enumerate(seq):
            before = np.full_like(a, FILL)
            d = dev(before)
            g.process(dev(a), d, mode, pattern)
            same_whole(host(d), wants[f], before, h, "blurzoom pal=%d mode=%d pattern=%d width %d frame %d" % (pal, mode, pattern, w, f))
    finally:
        g.close()


# blurzoom's buffer is the width rounded down to whole blocks of 32 pixels, so the buffer kernels cross their workgroup at the same widths as the frame kernels
for _pal, _mode, _pattern in ((3, 0, 0), (4, 1, 3)):
    for _w in sorted(set(widths(K_BZV, lo=32)[0] + widths(K_BZB, g=32, lo=32)[0] + [32, 33, 63, 64, 65])):
        add("blurzoom", "k_bz", run_blurzoom, _pal, _mode, _pattern, _w)
FORMS["blurzoom"] = {"k_bz"}


# ---- fused.hip
K_GCK = ("fused.hip", "cdiv(width,248)")


def run_gauss5_colorkey(orc, gpu, tune, form, ps, key, w, n=1):
    """key = 0: lgpu_gauss5 (aligned frames: the fused kernel with the key off); key = 1: lgpu_gauss5_colorkey, n > 1 through lgpu_fx_batch"""
    h = SPANS[K_GCK].rows
    rng = seeded("gck", ps, key, w, n)
    st = align(w * ps + 16)
    assert ta.rule_two("gauss5_colorkey", ps, st) == form and (w & 3) == 0
    col = (128, 120, 135)
    s1 = [src_frame(rng, w, h, ps, st) for _ in range(n)]
    for a in s1:
        a[:h, :w * ps] = (a[:h, :w * ps] >> 3) + 112           # near the key colour, so that the key fires on part of the frame
    s2 = [src_frame(rng, w, h, ps, st) for _ in range(n)]
    before = blank(h, st)
    wants = []
    for f in range(n):
        wt = before.copy()
        if key:
            bl = np.zeros_like(s1[f])
            orc.orc_gauss5(P(s1[f]), st, P(bl), st, w, h, ps)
            (orc.orc_colorkey if ps == 3 else orc.orc_colorkey4)(P(bl), st, P(s2[f]), st, P(wt), st, w, h, 1, 0.4, 0.7, *(col + ((0,) if ps == 3 else ())))
        else:
            orc.orc_gauss5(P(s1[f]), st, P(wt), st, w, h, ps)
        wants.append(wt)
    kept(h, *[(wt, before) for wt in wants])
    if gpu is None:
        return
    d1, d2, dd = [dev(a) for a in s1], [dev(a) for a in s2], [dev(before) for _ in range(n)]
    if n > 1:
        gpu.fx_batch(ta.FX["gauss5_colorkey"], [[t] for t in d1], [[t] for t in dd], w, h, ins1=[[t] for t in d2], ip=(ps, 1, col[0] | (col[1] << 8) | (col[2] << 16)), dp=(0.4, 0.7))
    elif key:
        gpu.gauss5_colorkey(d1[0], d2[0], dd[0], w, h, ps, 1, 0.4, 0.7, col)
    else:
        gpu.gauss5(d1[0], dd[0], w, h, psize=ps)
    for f in range(n):
        same_whole(host(dd[f]), wants[f], before, h, "gauss5%s ps=%d width %d frame %d" % (" + colorkey" if key else "", ps, w, f))


# strips of 248 columns, four of them to a workgroup: the widths of a strip and those of a workgroup; the fuzzer draws multiples of 4 from 4
GCK_W = sorted(set(both(K_GCK, g=4, lo=4, span=248) + widths(K_GCK, g=4, lo=4)[0]))
for _ps in (3, 4):
    for _key in (0, 1):
        for _w in GCK_W:
            add("gauss5_colorkey", "k_gauss5_colorkey<%d>" % _ps, run_gauss5_colorkey, _ps, _key, _w)
    add("gauss5_colorkey", "k_gauss5_colorkey<%d>" % _ps, run_gauss5_colorkey, _ps, 1, widths(K_GCK, g=4, lo=4)[0][1], 3)
FORMS["gauss5_colorkey"] = {"k_gauss5_colorkey<3>", "k_gauss5_colorkey<4>"}


ASKED_BY_CASES = frozenset(ASKED)


# ---------------------------------------------------------------------------------------------- the oracle against the live reference at the wide widths (CPU)
# tools/fuzz_oracle.py (tests/test_oracle_live.py) draws widths below 600, so the oracle these cases trust was never compared with the reference beyond a workgroup.
# family -> (rows, [(site, how widths() is asked)]): one comparison per wide width of the family's sites, at a geometry fixed through fuzz_oracle's Draw.fixed; every
# other choice of the case is drawn as ever, and fuzz_oracle.EXCEPTIONS stays in force (its `never` entries redraw those choices).  The `never` entries that
# concern a width -- odd widths of the subsampled targets (k4: the entry point refuses them) and rows too short for whole triples (deinterlace, deinterlace.c:45-308)
# -- exclude the same widths and pitches above: g = 2 in the rgb_to_yuv cases, the pitch of run_deinterlace.
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_oracle as fo  # noqa: E402

needs_ref = pytest.mark.skipif(not po.have_ref(), reason="oracle/_ref not built (oracle/ref/build_ref.sh needs the reference tree)")
LIVE = {
    "k1": (3, [(K_SWZ, {}), (K_ROW, {})]),
    "k2": (6, [(K_K2, dict(g=2, lo=2)), (K_K2S, dict(g=2, lo=2))]),
    "k2_lut16": (6, [(K_K2, dict(g=2, lo=2))]),
    # (the table counts bytes: the widths of 3- and of 4-byte pixels, both, since the family draws the pixel size)
    "k6": (3, [(K_GAM, dict(g=3, lo=6), 3), (K_GAM, dict(g=4, lo=8), 4), (K_GAMB, dict(g=3, lo=6), 3), (K_GAMB, dict(g=4, lo=8), 4)]),
    "k3": (3, [(K_K3, dict(g=2, lo=2)), (K3S["k_yuv444_to_rgb_s"], {})]),
    "k4": (4, [(K_K4, dict(g=2, lo=2)), (K4S["444"], {})]),
    "k4_lut16": (4, [(K_K4, dict(g=2, lo=2))]),
    "repack": (4, [(K_RPK, dict(g=2, lo=2)), (RPK_S["k_swab_s"], {}), (RPK_S["k_combine_s"], {})]),
    "repack411": (4, [(K_411, dict(g=4, lo=4))]),
    "chroma_up": (4, [(K_CUP, dict(g=2, lo=2))]),
    "yuv411_to_rgb": (3, [(K_411R, dict(g=4, lo=4))]),
    "rgb_to_yuv411": (3, [(K_411, dict(lo=4))]),
    "blend_chroma": (3, [(K_PIX2, {}), (K_ROW2, {})]),
    "blend_luma": (3, [(K_PIX2, {})]),
    "blend_multi": (3, [(K_PIX2, {})]),
    "colorkey": (3, [(K_PIX2, {})]),
    "mirror": (4, [(K_MIR4, {}), (K_ROW2, {})]),
    "softlight": (4, [(K_SOFTS, dict(g=4, lo=8)), (K_TILE, dict(g=2, lo=4))]),
    "edge": (6, [(K_EMAP4, dict(g=4, lo=8)), (K_TILE, dict(lo=4)), (K_EPAINT, dict(lo=4))]),
    "transition": (5, [(K_TRANS, dict(lo=2))]),
    "dissolve": (3, [(K_COL, {})]),
    "slide_over": (3, [(K_COL, {})]),
    "deinterlace": (6, [(K_DEINT, {})]),
    "script_fx": (3, [(K_LUTS, {})]),
    "triple_split": (3, [(K_COL, {})]),
    "compositor": (5, [(K_COMP, {})]),
    "blurzoom": (8, [(K_BZV, dict(lo=32)), (K_BZB, dict(g=32, lo=32))]),          # (blurzoom.c takes 8 rows and up)
    "rgbdelay": (3, [(K_RGBD, {}), (K_RGBD4, dict(g=4, lo=4))]),
}
NO_GEOMETRY = {"gamma_lut8", "gamma_lut16", "clamp_tables", "premult_tables", "get_resizable"}           # tables and planner questions: no frame


def live_widths(family):
    """the wide widths of the family's sites in pixels; a third entry is the bytes per pixel where the table counts bytes"""
    return sorted({w // (e[2] if len(e) > 2 else 1) for e in LIVE[family][1] for w in widths(e[0], **e[1])[0]})


def test_live_table_names_every_family():
    assert set(LIVE) | NO_GEOMETRY == set(fo.FAMILIES) and not set(LIVE) & NO_GEOMETRY
    for family in LIVE:
        assert 3 <= len(live_widths(family)) <= 12, family


_live = {}


@needs_ref
@pytest.mark.parametrize("family", list(LIVE))
def test_oracle_equals_the_live_reference_at_the_wide_widths(family):
    """the oracle and the reference build of the same operation, whole buffers, at each wide width of the family's launch sites"""
    if not _live:
        _live["ref"], _live["subject"] = fo.Ref(), fo.OracleSubject()
    h = LIVE[family][0]
    for k, w in enumerate(live_widths(family)):
        x = fo.Ctx(np.random.default_rng([20261019, k]), _live["ref"], _live["subject"], geometry=(w, h))
        try:
            fo.FAMILIES[family](x)
        except (fo.Mismatch, fo.Refused) as e:
            raise AssertionError("%s at %d x %d: %s" % (family, w, h, e))
        assert x.overmasked == 0


# ---------------------------------------------------------------------------------------------- the tests
@G
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_wide(gpu, orc, tune, case):
    """one case on the device: the kernel's output over the whole allocation against the oracle's"""
    group, form, fn, args = case
    if group == "edge":
        tune("EDGE_NO_S", 0)
    fn(orc, gpu, tune, form, *args)


def _notune(name, value):
    raise AssertionError("the oracle-only pass must not touch the library")


def test_oracle_accepts_every_case(orc):
    """every case of this module without a device: inputs, oracle, guard bytes and the restated form; a case that no longer reaches the form it names fails here"""
    for group, form, fn, args in CASES:
        try:
            fn(orc, None, _notune, form, *args)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (case_id((group, form, fn, args)), e))


def test_cases_reach_their_forms():
    """every group of cases reaches, between its cases, each kernel form its dispatcher can choose -- and names no other"""
    assert set(FORMS) == {c[0] for c in CASES}
    for group, forms in FORMS.items():
        named = {c[1] for c in CASES if c[0] == group}
        assert named == forms, "%s: the cases name %s, the dispatcher can choose %s" % (group, sorted(named), sorted(forms))
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids), "case ids repeat: %s" % [i for i, k in collections.Counter(ids).items() if k > 1][:5]


def case_arg(c, name):
    """the argument of a case that its run function calls `name`"""
    return c[3][list(inspect.signature(c[2]).parameters)[4:].index(name)]


def test_cell_sweeps_include_a_row_of_one_cell():
    """every kernel that splits a linear cell index with a magic division (its host code corrects the magic at ngr == 1) runs on a frame whose rows are ONE cell, and on
    rows of 511, 512, 513 and 1025 cells"""
    for key, e in SPANS.items():
        if not e.linear:
            continue
        kernel = key[1].split(":")[1]
        mine = [c for c in CASES if c[1] == kernel]
        if key == K_K2S:
            for nc in (1, 2, 4):
                cells = {((case_arg(c, "w") >> 1) + nc - 1) // nc for c in mine if case_arg(c, "nc") == nc}
                assert {1, 511, 512, 513, 1025} <= cells, "%s NC=%d: rows of %s cells" % (kernel, nc, sorted(cells))
            continue
        cells = {case_arg(c, "w") // e.unit for c in mine}
        assert {1, 2, 511, 512, 513, 1025} <= cells, "%s: rows of %s cells" % (kernel, sorted(cells))


def test_every_site_has_cases():
    """the case lists above asked widths() for every launch site of SPANS (recorded when the lists were built, before anything else calls it): a site added to the
    table whose widths no case takes fails here"""
    assert ASKED_BY_CASES == set(SPANS), "sites no case takes its widths from: %s" % sorted(set(SPANS) - ASKED_BY_CASES)
