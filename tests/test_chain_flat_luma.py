"""lgpu_chain_flat_yuv_luma (include/lives_gpu_luma.h): a luma overlay -- overlay, underlay, negative overlay, averaged overlay of simple_blend.c -- between two decoded
frames of any of the four decoded formats as ONE launch that converts the keyed layer everywhere and the other layer only in waves that show some of it, against the
oracle's composition of the header's definition, step by step: layer 2 through the single-frame conversion of its format (tests/test_chain_flat_mix422.py's to_rgba),
layer 1 the same way [-> orc_swizzle], [both letterboxed onto opaque black: tests/test_chain_flat_select.py's letterboxed], orc_blend_luma(type, A, B, dst = A, psize 4,
pal_order = the chain's order, threshold, inplace = 1) at the canvas's size or the frame's, [orc_gamma_apply], [orc_rgb_to_yuv].  Bit-exact: every byte of every
destination plane, and every byte of the planes' row padding and guard rows.  At size also against the device's own staged launches, at threshold 0 against layer 1's
single-layer flat form; and the refusals.

A pair is written (layer 1's format, layer 2's format).  The KEYED layer is the one whose luma decides: layer 2 for type 2, layer 1 for types 1, 3 and 4; the kernel
calls it K and the other one O.

Every GPU case is a `spec` made by one of the *_specs() generators below, which the CPU test of the premises walks too: each track's selection map (the oracle's output
compared pixel-wise with A and with B) shows BOTH layers unless the case is named as an end.  The thresholds are CHOSEN to hold this (choose_thresholds: per track the
first value of one fixed shuffled list that does, by the oracle alone).  The structured case carries one more premise: cut into the kernel's waves -- 64 consecutive
chroma columns of a unit's rows -- its map holds a wave that shows only K, one that shows only O and a mixed one, for every type."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.offset_buffers import dev_at
from tests.test_chain_flat import UNIT_CAP, gamma_lut, plane_dims
from tests.test_chain_flat_mix422 import (E_BADARG, E_UNSUPPORTED, GUARD, NAME, PAIRS, PIXBUF, NOBLEND, UYVY, YUYV, YUV420P, YUV422P, RGBA, case, layer, pair_id, packed,
                                          source_of, to_rgba, up)
from tests.test_chain_flat_select import INVERTED, clips, figure_of, letterboxed, pair_layers, plane_size, with_lut
from tests.util import align, host

P = po.P
OVERLAY, UNDERLAY, NEGATIVE, AVERAGED = 1, 2, 3, 4
TYPES = [OVERLAY, UNDERLAY, NEGATIVE, AVERAGED]
TYPE_NAME = {OVERLAY: "overlay", UNDERLAY: "underlay", NEGATIVE: "negative overlay", AVERAGED: "averaged overlay"}
SMALL = [(2, 1), (2, 2), (2, 3), (4, 2), (6, 5)]
SMALL_PAIRS = [(YUV420P, YUV420P), (YUV422P, UYVY)]        # YUV420P over YUV420P, UYVY over YUV422P
FMTS = [RGBA, UYVY, YUYV, YUV420P]
DARK, BRIGHT, BLOCK = 40, 200, 128                         # the structured case: luma samples of its two constant blocks, and their width in pixels (one wave: 64 cells)
STRUCTURED = (388, 6)                                      # 194 cells a row: waves of 64, 64, 64 and 2 lanes -- the dark block, the bright block, noise, noise


def keyed(type_):
    """the layer whose luma decides (luma_pred.h, luma_keyed_layer)"""
    return 2 if type_ == UNDERLAY else 1


# ---- the oracle's side ----------------------------------------------------------------------------------------------------------------------------------------------
def layers_rgba(orc, s, i):
    """steps 1 to 3 of the header for track i of spec s: (A, B, width, height), both in the chain's byte order, canvas-sized on a canvas"""
    c, canvas, order, swap = s["c"], s["canvas"], s["order"], s["swap"]
    f1, f2, sw, sh = c["f1"], c["f2"], c["sw"], c["sh"]
    B = to_rgba(orc, f2, c["frames2"][i], sw, sh, order ^ swap, c["L2"])
    A = to_rgba(orc, f1, c["frames"][i], sw, sh, order, c["L1"])
    if swap:
        sw_ = np.zeros((sh, sw * 4), np.uint8)
        orc.orc_swizzle(po.OPS.index("swap3postalpha"), 0, P(A), sw * 4, P(sw_), sw * 4, sw, sh, None)
        A = sw_
    if canvas:
        return letterboxed(orc, A, sw, sh, canvas), letterboxed(orc, B, sw, sh, canvas), canvas[0], canvas[1]
    return A, B, sw, sh


def luma_oracle(orc, type_, A, B, w, h, pal_order, thresh):
    """step 4: lgpu_blend_luma(type, A, B, dst = A, psize 4, pal_order, thresh) as the oracle has it, in place on a copy of A"""
    out = A.copy()
    orc.orc_blend_luma(type_, P(out), out.strides[0], P(B), B.strides[0], P(out), out.strides[0], w, h, 4, pal_order, int(thresh), 1)
    return out


def expected_luma(orc, s, i, thresh=None):
    """the six steps for track i of spec s: the list of destination planes"""
    c, fmt, order, swap = s["c"], s["fmt"], s["order"], s["swap"]
    A, B, w, h = layers_rgba(orc, s, i)
    out = luma_oracle(orc, s["type"], A, B, w, h, order ^ swap, s["thresholds"][i] if thresh is None else thresh)
    lut = s["lut"]
    if lut is not None:
        orc.orc_gamma_apply(P(out), w * 4, w, h, 4, 0, P(lut))
    if fmt == RGBA:
        return [out]
    want, _ = po.k4_out_planes(0, c["sw"], c["sh"], fmt, 0)
    wp, ws = po.planes_args(want)
    assert orc.orc_rgb_to_yuv(P(out), out.strides[0], c["sw"], c["sh"], order ^ swap, 1, ctypes.addressof(wp), ctypes.addressof(ws), fmt, 0, s["wt_sink"]) == 0
    return want


def sel_map(orc, type_, A, B, w, h, pal_order, thresh, frame=None):
    """the selection map of the frame's pixels: the oracle's output compared pixel-wise with A and with B.  (shows2, shows1): where the output is B's pixel and not A's,
    and the reverse; a pixel that is the same in both layers is in neither.  frame = (ox, oy, sw, sh) on a canvas"""
    out = luma_oracle(orc, type_, A, B, w, h, pal_order, thresh).reshape(h, w, 4)
    a, b = A.reshape(h, w, 4), B.reshape(h, w, 4)
    is_a, is_b = (out == a).all(axis=2), (out == b).all(axis=2)
    assert (is_a | is_b).all(), "a pixel of the overlay is neither layer's"
    ox, oy, sw, sh = frame or (0, 0, w, h)
    cut = lambda m: m[oy:oy + sh, ox:ox + sw]
    return cut(is_b & ~is_a), cut(is_a & ~is_b)


def waves_of(shows_o, shows_k):
    """the map cut into the kernel's waves: the units of K2's walk (row 0, the row pairs from row 1, the trailing row of an even height) x 64 consecutive chroma
    columns inside a workgroup of 256.  A list of "K" (every pixel shows K), "O" (every pixel shows O) or "mixed"; every pixel of the map must be decided"""
    sh, sw = shows_o.shape
    assert (shows_o ^ shows_k).all(), "a pixel is the same in both layers: its wave cannot be told from the output"
    npairs = (sh - 1) // 2
    units = [(0, 1)] + [(2 * u - 1, 2 * u + 1) for u in range(1, npairs + 1)] + ([(sh - 1, sh)] if (sh - 1) & 1 else [])
    out = []
    for r0, r1 in units:
        for g0 in range(0, sw // 2, 256):
            for c0 in range(g0, min(g0 + 256, sw // 2), 64):
                o = shows_o[r0:r1, 2 * c0:2 * min(c0 + 64, g0 + 256, sw // 2)]
                out.append("O" if o.all() else "mixed" if o.any() else "K")
    return out


CANDIDATES = [int(k) + 1 for k in np.random.default_rng(0x10AA).permutation(255)]          # 1 .. 255 in one fixed shuffled order


def holds(orc, s, i, t):
    """the premises of track i at threshold t, as a dict of booleans (every one must be True).  both: the frame shows both layers; waves (the structured case): a wave
    of each kind"""
    A, B, w, h = layers_rgba(orc, s, i)
    c = s["c"]
    fw, fh, ox, oy = figure_of(c["sw"], c["sh"], s["canvas"])
    two, one = sel_map(orc, s["type"], A, B, w, h, s["order"] ^ s["swap"], t, (ox, oy, c["sw"], c["sh"]))
    out = {"both": bool(two.any() and one.any())}
    if s["structured"]:
        undecided = not (two ^ one).all()
        kinds = set() if undecided else set(waves_of(*((one, two) if keyed(s["type"]) == 2 else (two, one))))
        out["waves"] = kinds == {"K", "O", "mixed"}
    return out


def choose_thresholds(orc, s):
    """distinct thresholds, track t's the first unused candidate that holds every premise"""
    out, used = [], set()
    for i in range(s["c"]["ntracks"]):
        for t in CANDIDATES:
            if t not in used and all(holds(orc, s, i, t).values()):
                used.add(t)
                out.append(t)
                break
        else:
            raise AssertionError("no threshold holds the premises: %s, track %d" % (what(s), i))
    return out


def structure(f, fr, sw, sh):
    """the structured case's keyed layer: the frame's first 128 pixels of every row a constant dark luma, the next 128 a constant bright one, chroma 128 under both;
    the rest stays the noise that was drawn"""
    pl, st = fr
    if packed(f):
        m = pl[0][:, :sw * 2].reshape(sh, sw // 2, 4)
        yi, ci = ((1, 3), (0, 2)) if f == UYVY else ((0, 2), (1, 3))
        for k, v in enumerate((DARK, BRIGHT)):
            for j in yi:
                m[:, k * BLOCK // 2:(k + 1) * BLOCK // 2, j] = v
            for j in ci:
                m[:, k * BLOCK // 2:(k + 1) * BLOCK // 2, j] = 128
    else:
        pl[0][:, :BLOCK], pl[0][:, BLOCK:2 * BLOCK] = DARK, BRIGHT
        for k in (1, 2):
            pl[k].reshape(-1, st[k])[:, :2 * BLOCK // 2] = 128          # the chroma columns of both blocks


def spec(orc, seed, pair, sw, sh, type_, fmt=RGBA, ntracks=2, canvas=None, thresholds=None, ends=False, lut=None, order=0, swap=0, L1=None, L2=None, wt_sink=0, yvu_sink=False,
         pads=(8, 3, 5), dst_off=0, l1_offs=None, l2_offs=None, structured=False):
    """one GPU case: the frames (tests/test_chain_flat_mix422.py's case()) and the thresholds (chosen to hold the premises unless given; ends: they are given and the map
    is single-layer).  structured: the keyed layer carries the dark and the bright block (structure())"""
    f1, f2 = pair
    seed = [int(v) for v in np.atleast_1d(seed)]
    c = case(seed, f1, f2, sw, sh, fmt, ntracks=ntracks, L1=L1, L2=L2, amounts=[0] * ntracks)
    if structured:
        for i in range(ntracks):
            structure(f2 if keyed(type_) == 2 else f1, (c["frames2"] if keyed(type_) == 2 else c["frames"])[i], sw, sh)
    s = dict(c=c, seed=seed, type=type_, fmt=fmt, canvas=canvas, thresholds=thresholds, ends=ends, lut=lut, order=order, swap=swap, wt_sink=wt_sink, yvu_sink=yvu_sink, pads=pads,
             dst_off=dst_off, l1_offs=l1_offs, l2_offs=l2_offs, structured=structured)
    if thresholds is None:
        s["thresholds"] = choose_thresholds(orc, s)
    assert len(s["thresholds"]) == ntracks
    return s


def what(s):
    c = s["c"]
    return "%s, %s over %s, %dx%d%s, fmt %d" % (TYPE_NAME[s["type"]], NAME[c["f2"]], NAME[c["f1"]], c["sw"], c["sh"], " on %s" % (s["canvas"],) if s["canvas"] else "", s["fmt"])


# ---- the device's side -----------------------------------------------------------------------------------------------------------------------------------------------
def run(gpu, orc, s):
    """one call with tracks that all differ; the device buffers are allocated in a shuffled order and handed over in another (slot order != frame order); every
    destination plane is compared whole: frame bytes against the oracle, row padding and guard rows against their fill"""
    ops = gpu
    c, canvas, fmt, order, swap = s["c"], s["canvas"], s["fmt"], s["order"], s["swap"]
    f1, f2, sw, sh, n = c["f1"], c["f2"], c["sw"], c["sh"], c["ntracks"]
    rng = np.random.default_rng(s["seed"] + [3])
    fw, fh, _, _ = figure_of(sw, sh, canvas)
    dims = plane_dims(fmt, fw, fh)
    pads = s["pads"]
    strides = [align(b + pads[k], 4 if fmt in (RGBA, UYVY, YUYV) else 2 if k == 0 else 1) for k, (b, _) in enumerate(dims)]
    fills = [[rng.integers(0, 256, (r + GUARD, strides[k]), dtype=np.uint8) for k, (_, r) in enumerate(dims)] for _ in range(n)]
    d1, d2, d_pl = [None] * n, [None] * n, [None] * n
    l1_offs, l2_offs = s["l1_offs"], s["l2_offs"]
    for i in rng.permutation(n):
        d_pl[i] = [dev_at(f, s["dst_off"] if k == 0 else 0) for k, f in enumerate(fills[i])]
        d2[i] = [up(p, l2_offs[j] if l2_offs else None) for j, p in enumerate(c["frames2"][i][0])]
        d1[i] = [up(p, l1_offs[j] if l1_offs else None) for j, p in enumerate(c["frames"][i][0])]
    slots = [int(k) for k in rng.permutation(n)]
    dsel = [0, 2, 1] if (s["yvu_sink"] and fmt == YUV420P) else list(range(len(dims)))
    prm = ops.chain_params(sw, sh, 0, sw, sh, 0, strides[0] if fmt == RGBA else 0, swap_rb=swap, interp=PIXBUF, bf=0, lut=s["lut"])
    src, src2 = source_of(ops, f1, c["frames"][0], c["L1"], order), source_of(ops, f2, c["frames2"][0], c["L2"], order ^ swap)
    sink = ops.chain_sink(fmt, [strides[j] for j in dsel], which_tables=s["wt_sink"], in_order=order ^ swap) if fmt != RGBA else None

    def chroma(d, f, j):
        return [d[k][j] for k in slots] if not packed(f) else None
    trk = ops.chain_yuv_mix_tracks([d1[k][0] for k in slots], chroma(d1, f1, 1), chroma(d1, f1, 2), [d2[k][0] for k in slots], chroma(d2, f2, 1), chroma(d2, f2, 2),
                                   [[d_pl[k][j] for j in dsel] for k in slots])
    ops.chain_flat_yuv_luma(prm, src, src2, trk, s["type"], np.array([s["thresholds"][k] for k in slots], np.uint8), sink=sink, canvas=canvas)
    wants = []
    for i in range(n):
        want = expected_luma(orc, s, i)
        wants.append(want)
        for p, j in enumerate(dsel):              # p: the conversion's plane (Y, U, V); j: the buffer it was handed
            b, r = dims[p]
            got = host(d_pl[i][j])
            bad = got[:r, :b] != want[p][:r, :b]
            assert not bad.any(), "%s, track %d (threshold %s) plane %d: %d bytes differ from the oracle, first at %s" % (
                what(s), i, s["thresholds"][i], p, int(bad.sum()), np.argwhere(bad)[0].tolist())
            assert (got[:r, b:] == fills[i][j][:r, b:]).all(), "%s, track %d plane %d: row padding was written" % (what(s), i, p)
            assert (got[r:] == fills[i][j][r:]).all(), "%s, track %d plane %d: guard rows were written" % (what(s), i, p)
    return wants


# ---- the case lists: generators of specs, walked by the GPU tests and by the CPU test of their premises ----------------------------------------------------------------
def small_specs(orc, sw, sh):
    """the walks' smallest frames: all four types, two pairs, all four destinations (the 4:2:0 sink on even heights)"""
    for p, pair in enumerate(SMALL_PAIRS):
        for type_ in TYPES:
            for fmt in FMTS:
                if fmt == YUV420P and sh & 1:
                    continue
                j = p + type_ + fmt
                L1, L2 = pair_layers(pair, j)
                yield spec(orc, [0x10A1, sw, sh, p, type_, fmt], pair, sw, sh, type_, fmt, ntracks=2, L1=L1, L2=L2, lut="gamma" if j & 1 else None, swap=j & 1, order=(j >> 1) & 1,
                           wt_sink=j & 1, pads=(2, 1, 3) if fmt == YUV420P else (8, 3, 5))


def pair_specs(orc, pair):
    """36x10: every pair of PAIRS, the types rotated with the pair, to RGBA and to one sink each; LUT, swap_rb, out_order, table sets, pb_quality, FIX_EDGES and the
    sink's tables and plane order move on with every case"""
    j = PAIRS.index(pair)
    for k, fmt in enumerate((RGBA, [UYVY, YUV420P, YUYV][j % 3])):
        type_ = TYPES[(j + k) % 4]
        L1, L2 = pair_layers(pair, j + k)
        yield spec(orc, [0x10A2, j, fmt], pair, 36, 10, type_, fmt, ntracks=2, L1=L1, L2=L2, lut=[None, "gamma", INVERTED][(j + k) % 3], order=(j >> 1) & 1, swap=(j + k) & 1,
                   wt_sink=(j % 4) if fmt == YUV420P else j & 1, yvu_sink=bool(j & 2), pads=(8 * (j & 1), 3, 5))


def edge_specs(orc):
    """516x5: 258 cells a row, two workgroups along x, the second with two lanes that own a cell: its other 254 exit before the vote"""
    for t, type_ in enumerate(TYPES):
        pair = [(UYVY, YUV422P), (YUV420P, YUYV), (YUV422P, YUV420P), (YUV420P, YUV420P)][t]
        yield spec(orc, [0x10A3, type_], pair, 516, 5, type_, [RGBA, UYVY][t & 1], ntracks=1, L1=layer(tight=True, pad=(0, 1, 1)), L2=layer(fix=1, pad=(4, 0, 3), tight=True),
                   lut="gamma", swap=t & 1)


def structured_specs(orc):
    """388x6: the keyed layer's dark block, bright block and noise make a wave that shows only O, one that shows only K and mixed ones, for every type; to RGBA and to
    YUV420P.  The keyed layer is YUV420P for the overlays and UYVY for the underlay"""
    sw, sh = STRUCTURED
    for type_ in TYPES:
        for fmt in (RGBA, YUV420P):
            pair = (YUV420P, UYVY) if type_ != AVERAGED else (YUV420P, YUV422P)
            yield spec(orc, [0x10A4, type_, fmt], pair, sw, sh, type_, fmt, ntracks=2, L1=layer(), L2=layer(wt=1), lut="gamma" if fmt == RGBA else None, swap=int(fmt == RGBA),
                       wt_sink=2 if fmt == YUV420P else 0, pads=(4, 1, 3), structured=True)


def track_specs(orc, ntracks):
    """6x4 with 33 and 64 tracks, distinct thresholds and frames on every track: 32 tracks per launch, so two launches"""
    for type_, fmt, pair in ((OVERLAY, RGBA, (UYVY, YUV422P)), (UNDERLAY, YUV420P, (YUV420P, UYVY)), (NEGATIVE, UYVY, (YUV422P, YUV420P))):
        yield spec(orc, [0x10A5, ntracks, type_], pair, 6, 4, type_, fmt, ntracks=ntracks, L1=layer(wt=1, pad=(4, 1, 3)), L2=layer(wt=0 if packed(pair[1]) else 2, pad=(0, 3, 1)),
                   lut="gamma", swap=ntracks & 1, wt_sink=int(fmt == YUV420P) * 2, yvu_sink=True)


CANVAS = (36, 10, (44, 14, 3, 1))


def canvas_specs(orc):
    """36x10 on 44x14 at (3, 1), not centred, under a LUT that does not keep black: a bar pixel is 255, 255, 255"""
    sw, sh, cv = CANVAS
    assert (cv[2], cv[3]) != ((cv[0] - sw + 1) >> 1, (cv[1] - sh + 1) >> 1)
    for t, type_ in enumerate(TYPES):
        pair = PAIRS[(2 * t + 1) % len(PAIRS)]
        L1, L2 = pair_layers(pair, t)
        yield spec(orc, [0x10A6, type_], pair, sw, sh, type_, RGBA, ntracks=2, canvas=cv, L1=L1, L2=L2, lut=INVERTED, swap=t & 1, order=(t >> 1) & 1, pads=(4 * t, 0, 0))


def address_specs(orc, dst_off):
    """the destination at 4 and 12 mod 16 with pitches of 4 mod 8 (4-byte stores where the address is no multiple of 8), the 4:2:0 luma plane at 2 mod 4; packed layers
    at 0, 4, 8 and 12 mod 16; planar layers' planes at odd addresses with odd pitches"""
    assert (132 * 4 + 4) % 8 == 4 and (132 * 2 + 4) % 8 == 4
    for n, off in enumerate((0, 4, 8, 12)):
        pair = [(YUV420P, UYVY), (YUV422P, YUYV), (YUYV, UYVY), (UYVY, YUYV)][n]
        l1_offs = (12 - off, 0, 0) if packed(pair[0]) else (1, 3, 5)
        for fmt, pads, doff in ((RGBA, (4, 0, 0), dst_off), (UYVY, (4, 0, 0), dst_off), (YUV420P, (2, 1, 1), dst_off + 2)):
            yield spec(orc, [0x10A7, dst_off, off, fmt], pair, 132, 8, TYPES[(n + fmt) % 4], fmt, ntracks=2, L1=layer(pad=(4, 1, 1)), L2=layer(pad=(4 * (n & 1), 0, 0), wt=1), pads=pads,
                       dst_off=doff, l1_offs=l1_offs, l2_offs=(off, 0, 0), lut="gamma" if fmt == RGBA else None)


def unit_specs(orc):
    """a frame of width 16 with more units than a launch has workgroup rows, so a workgroup walks a run of units on one staging of its tables"""
    tall = 2 * UNIT_CAP + 6
    assert -(-(tall // 2 + 1) // UNIT_CAP) == 2              # units per workgroup (flat_plan.h: ceil(nunits / cap))
    for t, (type_, pair, fmt) in enumerate(((NEGATIVE, (UYVY, YUV422P), RGBA), (UNDERLAY, (YUV420P, YUYV), YUV420P))):
        yield spec(orc, [0x10A8, t], pair, 16, tall, type_, fmt, ntracks=1, L1=layer(fix=1, pad=(4, 1, 1)), L2=layer(wt=1, pad=(0, 1, 0), tight=True), swap=1)


def end_specs(orc):
    """threshold 0: every type shows layer 1 everywhere (the oracle's word for it: test_every_gpu_case_holds_its_premises)"""
    for t, type_ in enumerate(TYPES):
        yield spec(orc, [0x10A9, type_], PAIRS[(3 * t) % len(PAIRS)], 36, 10, type_, [RGBA, UYVY, YUV420P, YUYV][t], ntracks=2, thresholds=[0, 0], ends=True, lut="gamma", swap=t & 1)


def all_spec_lists(orc):
    """every generator above with every parameter its GPU test runs it with: (name, generator)"""
    for sw, sh in SMALL:
        yield "small %dx%d" % (sw, sh), small_specs(orc, sw, sh)
    for pair in PAIRS:
        yield "pairs " + pair_id(pair), pair_specs(orc, pair)
    yield "workgroup edge", edge_specs(orc)
    yield "structured", structured_specs(orc)
    for n in (33, 64):
        yield "tracks %d" % n, track_specs(orc, n)
    yield "canvas", canvas_specs(orc)
    for off in (4, 12):
        yield "addresses %d" % off, address_specs(orc, off)
    yield "units", unit_specs(orc)
    yield "ends", end_specs(orc)


AT_SIZE_THRESHOLD = 64          # the threshold of the case at 1920x1080 (and of the benchmark)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_luma_symbol_struct_and_wrapper():
    """1. the entry point is in the built library under a prototype of its own table, lgpu_luma_key is laid out as include/lives_gpu_luma.h has it (int, pointer: 16
    bytes on LP64), the wrapper fills it, and neither lives_gpu.h nor lives_gpu_select.h declares anything of this form"""
    import os
    import re
    from lives_amd import lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "lives_gpu_luma.h")).read(), flags=re.S)
    assert re.findall(r"\b(lgpu_[a-z0-9_]+)\s*\(", text) == ["lgpu_chain_flat_yuv_luma"] and '#include "lives_gpu.h"' in text
    assert re.search(r"typedef struct \{\s*int type;\s*const uint8_t \*thresholds;\s*\} lgpu_luma_key;", text), "lgpu_luma_key is not laid out as the ctypes struct reads it"
    for other in ("lives_gpu.h", "lives_gpu_select.h"):
        assert "lgpu_chain_flat_yuv_luma" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", other)).read(), flags=re.S)
    assert "lgpu_chain_flat_yuv_luma" not in lib.PROTOTYPES and "lgpu_chain_flat_yuv_luma" not in lib.SELECT_PROTOTYPES
    assert len(lib.LUMA_PROTOTYPES["lgpu_chain_flat_yuv_luma"]) == 9
    K = lib.LumaKey
    assert ctypes.sizeof(K) == 16 and K.type.offset == 0 and K.thresholds.offset == 8
    L = lib.load()
    assert hasattr(L, "lgpu_chain_flat_yuv_luma") and L.lgpu_chain_flat_yuv_luma.argtypes == lib.LUMA_PROTOTYPES["lgpu_chain_flat_yuv_luma"]
    assert lib.LGPU_CHAIN_LUMA_TRACKS == 32
    k = ops.luma_key(3, [0, 64, 255])
    assert (k.type, k.thresholds[0], k.thresholds[1], k.thresholds[2]) == (3, 0, 64, 255)
    assert not ops.luma_key(1, None).thresholds
    assert callable(ops.chain_flat_yuv_luma)


def test_every_gpu_case_holds_its_premises(orc):
    """2. for every GPU case and every track of it: the selection map shows both layers -- unless the case is named as an end, and then every pixel that differs between
    the layers is layer 1's; the thresholds of a case are distinct; the structured case has a wave of each kind, for every type"""
    ncases, types = 0, set()
    for name, gen in all_spec_lists(orc):
        for s in gen:
            ts = s["thresholds"]
            for i, t in enumerate(ts):
                if s["ends"]:
                    A, B, w, h = layers_rgba(orc, s, i)
                    two, one = sel_map(orc, s["type"], A, B, w, h, s["order"] ^ s["swap"], t)
                    assert t == 0 and not two.any() and one.any(), "%s: %s track %d: threshold 0 is not layer 1 alone" % (name, what(s), i)
                    continue
                assert 1 <= t <= 255
                pr = holds(orc, s, i, t)
                assert all(pr.values()) and ("waves" in pr) == (name == "structured"), "%s: %s track %d, threshold %d: %s" % (name, what(s), i, t, pr)
            assert s["ends"] or len(set(ts)) == len(ts)
            if name == "structured":
                types.add(s["type"])
            ncases += 1
    assert ncases > 150 and types == set(TYPES)


def test_waves_of_cuts_as_the_kernel_walks():
    """3. the wave cut on maps whose answer is known: 388x6 has four units (row 0, two row pairs, the trailing row) of four waves each, the last two lanes wide; a
    column of O pixels at x = 129 makes the second wave of every unit mixed; 1030 pixels are three workgroups and nine waves a unit"""
    o = np.zeros((6, 388), bool)
    o[:, :128] = True
    assert waves_of(o, ~o) == ["O", "K", "K", "K"] * 4
    o[:, 129] = True
    assert waves_of(o, ~o) == ["O", "mixed", "K", "K"] * 4
    o[:] = False
    o[3, 386] = True                                          # the second row pair's upper row, the last wave
    assert waves_of(o, ~o) == ["K"] * 8 + ["K", "K", "K", "mixed"] + ["K"] * 4
    assert len(waves_of(np.zeros((1, 1030), bool), np.ones((1, 1030), bool))) == 9


def test_structured_frames_are_what_the_docstring_says(orc):
    """4. the structured case's keyed layer converts to a dark block, a bright block and noise: the keyed layer's luma plane (YUV420P) or luma samples (UYVY) are
    constant over each block, and the other layer is left as drawn"""
    for s in structured_specs(orc):
        c = s["c"]
        k2 = keyed(s["type"]) == 2
        f, frames = (c["f2"], c["frames2"]) if k2 else (c["f1"], c["frames"])
        for pl, st in frames:
            y = pl[0][:, 1:2 * STRUCTURED[0]:2] if f == UYVY else pl[0][:, :STRUCTURED[0]]
            assert (y[:, :BLOCK] == DARK).all() and (y[:, BLOCK:2 * BLOCK] == BRIGHT).all() and len(np.unique(y[:, 2 * BLOCK:])) > 64


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------------------
def go(gpu, orc, specs):
    n = 0
    for s in specs:
        run(gpu, orc, with_lut(orc, s))
        n += 1
    assert n


# The parts of the one GPU test at the end of this file.  Each walks its list as tests/test_chain_flat_select.py's tests do: a case is a call of a few milliseconds and
# every assertion names its case; all of them together run in about two seconds.
def luma_small_frames(gpu, orc):
    """5. row 0 alone, with and without a row pair and the trailing row, one and three cells wide (small_specs)"""
    for sw, sh in SMALL:
        go(gpu, orc, small_specs(orc, sw, sh))


def luma_pairs(gpu, orc):
    """6. all nine format pairs (pair_specs)"""
    for pair in PAIRS:
        go(gpu, orc, pair_specs(orc, pair))


def luma_waves(gpu, orc):
    """7. the workgroup edge, where the tail lanes exit before the vote (edge_specs), and the structured case, where whole waves skip the other layer
    (structured_specs)"""
    go(gpu, orc, edge_specs(orc))
    go(gpu, orc, structured_specs(orc))


def luma_tracks_canvas_and_units(gpu, orc):
    """8. 33 and 64 tracks as two launches (track_specs); the canvas under a LUT that does not keep black (canvas_specs); several units per workgroup (unit_specs)"""
    for n in (33, 64):
        go(gpu, orc, track_specs(orc, n))
    go(gpu, orc, canvas_specs(orc))
    go(gpu, orc, unit_specs(orc))


def luma_addresses(gpu, orc):
    """9. each alignment class the entry point and the kernel tell apart (address_specs)"""
    for dst_off in (4, 12):
        go(gpu, orc, address_specs(orc, dst_off))


def luma_threshold_0_is_layer_1s_single_form(gpu, orc):
    """10. the ends against the oracle (end_specs); then device against device at 644x38, UYVY over YUV420P, to RGBA and to UYVY: threshold 0 gives, for every type, the
    bytes of layer 1's single-layer flat form (lgpu_chain_flat_yuv420p[_to_yuv] with LGPU_INTERP_NOBLEND)"""
    import torch
    go(gpu, orc, end_specs(orc))
    ops = gpu
    w, h, n = 644, 38, 2
    lut = gamma_lut(orc)
    for fmt in (RGBA, UYVY):
        (A, st1), (B, st2) = clips(w, h, n, YUV420P, UYVY, 0xE2D + fmt)
        dims = plane_dims(fmt, w, h)
        new = lambda fill: [[torch.full((r, b), fill, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
        sink = ops.chain_sink(fmt, [b for (b, _) in dims], which_tables=0, in_order=1) if fmt != RGBA else None
        prm = ops.chain_params(w, h, 0, w, h, 0, w * 4, swap_rb=1, interp=PIXBUF, bf=0, lut=lut)
        s1 = ops.yuv_layer_source(YUV420P, st1, plane_size(A, 1), plane_size(A, 2), out_order=0, which_tables=1, pb_quality=2)
        s2 = ops.yuv_layer_source(UYVY, st2, 0, 0, out_order=1, which_tables=0, pb_quality=2)
        alone = new(0xC5)
        flat = ops.chain_params(w, h, 0, w, h, 0, w * 4, swap_rb=1, interp=PIXBUF | NOBLEND, bf=0, lut=lut)
        src1 = ops.yuv_source(st1, plane_size(A, 1), plane_size(A, 2), out_order=0, which_tables=1, pb_quality=2)
        if fmt == RGBA:
            ops.chain_flat_yuv420p(flat, src1, ops.chain_yuv_tracks(A[0], A[1], A[2], None, [t[0] for t in alone]), None)
        else:
            ops.chain_flat_yuv420p_to_yuv(flat, src1, sink, ops.chain_yuv_sink_tracks(A[0], A[1], A[2], None, alone), None)
        for type_ in TYPES:
            out = new(0x5C)
            ops.chain_flat_yuv_luma(prm, s1, s2, ops.chain_yuv_mix_tracks(A[0], A[1], A[2], B[0], None, None, out), type_, [0] * n, sink=sink)
            torch.cuda.synchronize()
            for t in range(n):
                for p in range(len(dims)):
                    assert torch.equal(out[t][p], alone[t][p]), "%s at threshold 0, fmt %d, track %d plane %d: %d bytes differ from layer 1's single-layer form" % (
                        TYPE_NAME[type_], fmt, t, p, int((out[t][p] != alone[t][p]).sum()))


def luma_at_1920x1080(gpu, orc):
    """11. 2 x 1920x1080, the underlay (the keyed layer is layer 2), YUV420P over UYVY to UYVY at threshold 64: byte-identical to the device's own staged launches on the
    same inputs -- the two conversions, lgpu_swizzle, lgpu_blend_luma in place, lgpu_gamma_apply, lgpu_rgb_to_yuv"""
    import torch
    from lives_amd import lib
    ops = gpu
    type_, (f1, f2), fmt = UNDERLAY, (UYVY, YUV420P), UYVY
    w, h, n = 1920, 1080, 2
    (A, st1), (B, st2) = clips(w, h, n, f1, f2, 0xA75)
    lut = gamma_lut(orc)
    dims = plane_dims(fmt, w, h)
    fused = [[torch.full((r, b), 0x5C, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
    today = [[torch.full((r, b), 0xC5, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
    sink = ops.chain_sink(fmt, [b for (b, _) in dims], which_tables=0, in_order=1)
    prm = ops.chain_params(w, h, 0, w, h, 0, w * 4, swap_rb=1, interp=PIXBUF, bf=0, lut=lut)
    s1 = ops.yuv_layer_source(f1, st1, 0, 0, out_order=0, which_tables=0, pb_quality=2)
    s2 = ops.yuv_layer_source(f2, st2, plane_size(B, 1), plane_size(B, 2), out_order=1, which_tables=0, pb_quality=3, flags=1)
    ops.chain_flat_yuv_luma(prm, s1, s2, ops.chain_yuv_mix_tracks(A[0], None, None, B[0], B[1], B[2], fused), type_, [AT_SIZE_THRESHOLD] * n, sink=sink)
    for t in range(n):
        a, a2, b = (torch.zeros((h, w * 4), dtype=torch.uint8, device="cuda") for _ in range(3))
        ops.yuv420p_to_rgb(B[0][t], B[1][t], B[2][t], b, w, h, 4, 1, 0, 0, 3, flags=1)
        ops.yuv_to_rgb([A[0][t]], a, w, h, f1, 0, 0, 1, 0)
        ops.swizzle(lib.SWAP3POSTALPHA, a, a2, w, h)
        ops.blend_luma(type_, a2, b, a2, w, h, 4, 1, AT_SIZE_THRESHOLD)
        ops.gamma_apply(a2, w, h, 4, lut)
        ops.rgb_to_yuv(a2, today[t], w, h, 1, 1, fmt, 0, 0)
    torch.cuda.synchronize()
    for t in range(n):
        for p in range(len(dims)):
            assert torch.equal(fused[t][p], today[t][p]), "track %d plane %d: %d bytes differ from today's launches" % (t, p, int((fused[t][p] != today[t][p]).sum()))
    assert not bool((fused[0][0] == 0x5C).all())


def luma_refusals(gpu, orc):
    """12. the refusals, for three format pairs (refusals_of)"""
    for pair in ((YUV422P, UYVY), (YUYV, YUV420P), (YUV420P, YUV422P)):
        refusals_of(gpu, pair)


def refusals_of(gpu, pair):
    """12. every LGPU_E_BADARG and LGPU_E_UNSUPPORTED item of the entry point -- the select form's, with the key's in place of the select's -- one call each: the code is
    compared and the destinations' fill is still whole afterwards; the same call inside the form then runs"""
    import torch
    from lives_amd import lib
    ops = gpu
    f1, f2 = pair
    w, h = 64, 36
    CW, CH = w + 16, h + 8

    def planes(f, y, u, v):
        if packed(f):
            return [torch.full((h, w * 2), y, dtype=torch.uint8, device="cuda"), None, None], (w * 2, 0, 0)
        ch = h // 2 if f == YUV420P else h
        return [torch.full((h, w), y, dtype=torch.uint8, device="cuda")] + [torch.full((ch, w // 2), c, dtype=torch.uint8, device="cuda") for c in (u, v)], (w, w // 2, w // 2)
    (A, full1), (B, full2) = planes(f1, 0, 0, 0), planes(f2, 200, 90, 160)
    orow0 = CW * 4 + 32
    D = [torch.full((CH + 8, orow0), 0x5C, dtype=torch.uint8, device="cuda") for _ in range(3)]
    csize = lambda pl: 0 if pl[1] is None else pl[1].numel()
    ptr = lambda t: None if t is None else t.data_ptr()

    def call(fmt=RGBA, canvas=None, type_=OVERLAY, thresholds=(64,), no_key=False, sw_=w, sh_=h, dw_=None, dh_=None, interp=PIXBUF, blur=0, ntracks=1, null=None, strides=full1,
             strides2=full2, usz=None, usz2=None, order=0, order2=None, swap=0, wt_src=0, wt_src2=0, q=2, q2=2, flags2=0, wt=0, in_order=None, orow=None, dst_off=0, in_place=None,
             in_fmt=f1, in_fmt2=f2, off2=0, no_src2=False):
        dw_, dh_ = sw_ if dw_ is None else dw_, sh_ if dh_ is None else dh_
        orow = orow if orow is not None else [orow0] * 3
        prm = ops.chain_params(sw_, sh_, 0, dw_, dh_, 0, orow[0], swap_rb=swap, interp=interp, do_blur=blur, bf=0)
        src = ops.yuv_layer_source(in_fmt, strides, csize(A) if usz is None else usz, csize(A), out_order=order, which_tables=wt_src, pb_quality=q)
        src2 = ops.yuv_layer_source(in_fmt2, strides2, csize(B) if usz2 is None else usz2, csize(B), out_order=(order ^ swap) if order2 is None else order2,
                                    which_tables=wt_src2, pb_quality=q2, flags=flags2)
        sink = ops.chain_sink(fmt, orow, which_tables=wt, in_order=(order ^ swap) if in_order is None else in_order) if fmt != RGBA else None
        m = max(ntracks, 1)
        trk = (lib.ChainYuvMixTrack * m)()
        for t in trk:
            t.y_d, t.u_d, t.v_d = ptr(A[0]), ptr(A[1]), ptr(A[2])
            t.y2_d, t.u2_d, t.v2_d = ptr(B[0]) + off2, ptr(B[1]), ptr(B[2])
            for k in range(3):
                t.dst_d[k] = D[k].data_ptr() + (dst_off if k == 0 else 0)
        if null == "dst":
            trk[0].dst_d[0] = None
        elif null is not None:
            setattr(trk[0], null, None)
        if in_place is not None:
            trk[0].dst_d[0] = (A + B)[in_place].data_ptr()
        if ntracks < 1:
            trk = (lib.ChainYuvMixTrack * 0)()
        th = list(thresholds) * m if thresholds is not None else None
        if no_key or no_src2:
            key = ops.luma_key(type_, th)
            cv = lib.Canvas(*canvas) if canvas else None
            return lib.load().lgpu_chain_flat_yuv_luma(ctypes.byref(prm), ctypes.byref(src), None if no_src2 else ctypes.byref(src2), None if no_key else ctypes.byref(key),
                                                       ctypes.byref(cv) if cv else None, ctypes.byref(sink) if sink else None, trk, len(trk), ops.stream_ptr())
        return ops.chain_flat_yuv_luma(prm, src, src2, trk, type_, th, sink=sink, canvas=canvas, check=False)

    cv0 = (CW, CH, 5, 3)
    badarg = {
        "type 0": dict(type_=0),
        "type 5": dict(type_=5),
        "type -1": dict(type_=-1),
        "null key": dict(no_key=True),
        "null thresholds": dict(thresholds=None),
        "a canvas and a sink": dict(fmt=UYVY, canvas=cv0),
        "canvas narrower than the frame": dict(canvas=(w - 2, CH, 0, 0)),
        "frame past the canvas's right edge": dict(canvas=(CW, CH, 17, 0)),
        "frame past the canvas's lower edge": dict(canvas=(CW, CH, 0, 9)),
        "negative offs_x": dict(canvas=(CW, CH, -1, 0)),
        "destination stride below the canvas row": dict(canvas=cv0, orow=[CW * 4 - 4] * 3),
        "destination stride below the row": dict(orow=[w * 4 - 4] * 3),
        "destination stride not a multiple of 4": dict(orow=[orow0 + 2] * 3),
        "destination not 4-byte aligned": dict(dst_off=2),
        "null destination": dict(null="dst"),
        "destination is layer 1's frame / luma plane": dict(in_place=0),
        "destination is layer 2's frame / luma plane": dict(in_place=3),
        "no PIXBUF": dict(interp=3),
        "no tracks": dict(ntracks=0),
        "65 tracks": dict(ntracks=65),
        "null src2": dict(no_src2=True),
        "in_fmt 1": dict(in_fmt=1),
        "src2 in_fmt 6": dict(in_fmt2=6),
        "null layer-1 frame / luma plane": dict(null="y_d"),
        "null layer-2 frame / luma plane": dict(null="y2_d"),
        "src2 out_order against the chain's (no swap)": dict(order=1, swap=0, order2=0),
        "src2 out_order against the chain's (swap)": dict(order=1, swap=1, order2=1),
        "source which_tables 4": dict(wt_src=4),
        "src2 which_tables -1": dict(wt_src2=-1),
        "pb_quality 0": dict(q=0),
        "src2 pb_quality 4": dict(q2=4),
        "src2 unknown flag": dict(flags2=2),
        "first stride below the row": dict(strides=(full1[0] - 4,) + full1[1:]),
        "src2 first stride below the row": dict(strides2=(full2[0] - 4,) + full2[1:]),
        "odd sw": dict(sw_=w - 1),
        "sh 0": dict(sh_=0),
        "sink out_fmt 1": dict(fmt=1),
        "sink in_order against the chain's": dict(fmt=UYVY, in_order=1),
        "sink which_tables 4": dict(fmt=YUV420P, wt=4),
        "BT.709 tables with a packed sink": dict(fmt=UYVY, wt=2),
        "sink stride below the row": dict(fmt=UYVY, orow=[w * 2 - 4] * 3),
    }
    unsupported = {
        "2:1": dict(dw_=w // 2, dh_=h // 2, orow=[orow0] * 3),
        "another width": dict(dw_=w + 2),
        "another height": dict(dh_=h - 1),
        "gaussian": dict(blur=1),
        "sink YUV422P": dict(fmt=5),
        "4:2:0 sink with an odd height": dict(fmt=YUV420P, sh_=h - 1),
        "packed sink at 2 mod 4": dict(fmt=UYVY, dst_off=2),
        "packed sink stride % 4 == 2": dict(fmt=YUYV, orow=[w * 2 + 2] * 3),
        "4:2:0 luma plane at an odd address": dict(fmt=YUV420P, dst_off=1),
        "4:2:0 luma stride odd": dict(fmt=YUV420P, orow=[w + 1, w, w]),
        "first plane of 2 GiB": dict(strides=(1 << 26, full1[1], full1[2])),
        "layer-2 first plane of 2 GiB": dict(strides2=(1 << 26, full2[1], full2[2])),
        "canvas-sized destination of 2 GiB": dict(canvas=cv0, orow=[1 << 26] * 3),
    }
    if packed(f1):
        badarg["BT.709 tables with a packed layer 1"] = dict(wt_src=2)
        unsupported["packed layer-1 rowstride % 4 == 2"] = dict(strides=(w * 2 + 2, 0, 0))
    else:
        badarg.update({"null U plane": dict(null="u_d"), "U plane one byte short": dict(usz=csize(A) - 1), "destination is layer 1's V plane": dict(in_place=2)})
        unsupported["U plane of 2 GiB"] = dict(usz=1 << 31)
    if packed(f2):
        badarg["BT.709 tables with a packed layer 2"] = dict(wt_src2=3)
        unsupported.update({"packed layer-2 rowstride % 4 == 2": dict(strides2=(w * 2 + 2, 0, 0)), "packed layer-2 plane at 2 mod 4": dict(off2=2)})
    else:
        badarg.update({"null layer-2 V plane": dict(null="v2_d"), "layer-2 U plane one byte short": dict(usz2=csize(B) - 1), "destination is layer 2's U plane": dict(in_place=4)})
        unsupported["layer-2 U plane of 2 GiB"] = dict(usz2=1 << 31)
    for want, table in ((E_BADARG, badarg), (E_UNSUPPORTED, unsupported)):
        for name, kw in table.items():
            for type_ in ((OVERLAY, UNDERLAY) if "type_" not in kw else (kw["type_"],)):          # the underlay changes the layers' places on the host: the refusals must not
                rc = call(**dict(kw, type_=type_))
                torch.cuda.synchronize()
                assert rc == want, "%s, type %d (%s): %d, expected %d (%s)" % (name, type_, kw, rc, want, lib.load().lgpu_last_error())
                assert all(bool((d == 0x5C).all()) for d in D), "%s: a destination was written" % name
    # ... and the same call inside the form runs: every type, to RGBA, onto the canvas and to both sinks; params->bf and LGPU_INTERP_NOBLEND are ignored
    for type_ in TYPES:
        assert call(type_=type_) == 0 and call(type_=type_, canvas=cv0) == 0 and call(type_=type_, interp=PIXBUF | NOBLEND) == 0
        torch.cuda.synchronize()
        assert bool((D[0][:CH, 3:CW * 4:4] == 255).all()) and bool((D[0][CH:] == 0x5C).all()) and bool((D[0][:, CW * 4:] == 0x5C).all())          # every pixel's alpha
        assert call(type_=type_, fmt=UYVY) == 0 and call(type_=type_, fmt=YUV420P, thresholds=(0,)) == 0 and call(type_=type_, thresholds=(255,)) == 0
        torch.cuda.synchronize()


PARTS = [luma_small_frames, luma_pairs, luma_waves, luma_tracks_canvas_and_units, luma_addresses, luma_threshold_0_is_layer_1s_single_form, luma_at_1920x1080, luma_refusals]


@pytest.mark.gpu
def test_luma_on_the_device(gpu, orc):
    """5 to 12, one after the other in one test: the parts are short and walk the same spec generators.  A failure names the part and, through the part's own
    assertion, the case"""
    for part in PARTS:
        try:
            part(gpu, orc)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (part.__name__, e)) from e
