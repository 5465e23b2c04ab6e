"""lgpu_chain_flat_yuv_select (include/lives_gpu_select.h): a select transition -- iris rectangle, iris circle, dissolve -- between two decoded frames of any of the
four decoded formats as ONE launch that converts only the layer a pixel shows, against the oracle's composition of the header's definition, step by step:
layer 2 through the single-frame conversion of its format (tests/test_chain_flat_mix422.py's to_rgba), layer 1 the same way [-> orc_swizzle], [both letterboxed onto
opaque black as tests/test_chain_flat422.py's oracle_tail does it], orc_transition / orc_dissolve (mask: orc_dissolve_mask) at the canvas's size or the frame's,
[orc_gamma_apply], [orc_rgb_to_yuv].  Bit-exact: every byte of every destination plane, and every byte of the planes' row padding and guard rows.  At size also
against the device's own launches, and at the two ends of a transition against each layer's single-layer flat form; and the refusals.

A pair is written (layer 1's format, layer 2's format).  Amount 1 shows layer 2 everywhere and amount 0 layer 1 -- but for the iris circle's centre: a pixel at the
figure's very centre (an even width, row height >> 1) has radius 0, the reference tests `radius > amount`, and 0 > 0 is false, so that one pixel shows layer 2 at
amount 0 too.  The circle at amount 0 is therefore no end: the figure sweep holds it to the oracle like every other amount.

Every GPU case is a `spec` made by one of the *_specs() generators below, which the CPU test of the premises walks too: each case's selection map (the oracle's
transition on an all-0x00 and an all-0xFF frame) shows BOTH layers unless the case is named as an end; on a canvas it differs from the map of the frame's own size and
origin; an iris's differs from the map computed with 3-byte pixels.  The amounts are CHOSEN to hold these (choose_amounts: the first candidates that do, by the oracle
alone).  One premise cannot hold and is replaced by what is true: the iris CIRCLE on a figure of even width has the same map at either pixel size -- its byte column
enters as (j - (wb >> 1)) / psize = x - width / 2 exactly -- so there the test asserts the equality, and the 3-byte premise is held by a canvas of odd width."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.offset_buffers import dev_at
from tests.test_chain_flat import UNIT_CAP, flat_planes, gamma_lut, plane_dims
from tests.test_chain_flat_mix422 import (E_BADARG, E_UNSUPPORTED, GUARD, NAME, PAIRS, PIXBUF, NOBLEND, UYVY, YUYV, YUV420P, YUV422P, RGBA, case, layer, pair_id, packed,
                                          source_of, to_rgba, up)
from tests.chain_ref import BLACK
from tests.util import align, host

P = po.P
RECT, CIRCLE, DISSOLVE = 0, 1, 3
KINDS = [RECT, CIRCLE, DISSOLVE]
KIND_NAME = {RECT: "rect", CIRCLE: "circle", DISSOLVE: "dissolve"}
INVERTED = (255 - np.arange(256)).astype(np.uint8)         # a LUT that does not keep black: a bar pixel is 255, 255, 255 under it
ALL_PAIRS = PAIRS + [(YUYV, UYVY), (YUV420P, YUYV)]
SMALL = [(2, 1), (2, 2), (2, 3), (4, 2), (6, 5)]
SMALL_PAIRS = [(YUV420P, YUV420P), (YUV422P, UYVY)]        # YUV420P over YUV420P, UYVY over YUV422P


# ---- the oracle's side ----------------------------------------------------------------------------------------------------------------------------------------------
def mask_of(orc, seed, w, h):
    m = np.zeros(w * h, np.float32)
    orc.orc_dissolve_mask(seed, w, h, m.ctypes.data)
    return m


def select_oracle(orc, kind, A, B, w, h, amount, mask, ps=4):
    """step 4: lgpu_transition(kind, A, B, .., ps, amount) / lgpu_dissolve(A, B, .., ps, mask, amount) as the oracle has them, into a tight frame"""
    out = np.zeros((h, w * ps), np.uint8)
    if kind == DISSOLVE:
        orc.orc_dissolve(P(A), A.strides[0], P(B), B.strides[0], P(out), w * ps, w, h, ps, mask.ctypes.data, float(amount))
    else:
        orc.orc_transition(kind, P(A), A.strides[0], P(B), B.strides[0], P(out), w * ps, w, h, ps, float(amount))
    return out


def sel_map(orc, kind, w, h, amount, mask, ps=4):
    """the selection map: True where the transition shows layer 2 -- the oracle's transition on an all-0x00 and an all-0xFF frame"""
    out = select_oracle(orc, kind, np.zeros((h, w * ps), np.uint8), np.full((h, w * ps), 0xFF, np.uint8), w, h, amount, mask, ps)
    px = out.reshape(h, w, ps)
    assert ((px == 0) | (px == 0xFF)).all() and (px == px[:, :, :1]).all()
    return px[:, :, 0] == 0xFF


def letterboxed(orc, rgba, sw, sh, canvas):
    """step 3: the frame onto opaque black, as tests/test_chain_flat422.py's oracle_tail does it (orc_letterbox where the frame is centred, the blit elsewhere)"""
    w, h, ox, oy = canvas
    big = np.zeros((h, w * 4), np.uint8)
    if (ox, oy) == ((w - sw + 1) >> 1, (h - sh + 1) >> 1):
        orc.orc_letterbox(P(rgba), sw * 4, sw, sh, P(big), w * 4, w, h, 4, P(BLACK))
    else:
        big[:, 3::4] = 255
        big[oy:oy + sh, ox * 4:(ox + sw) * 4] = rgba
    return big


def expected_select(orc, s, i, wrong2=False, mask=None):
    """the six steps of the header for track i of spec s: the list of destination planes.  wrong2: layer 2 read as the WRONG format (the mix tests' wrong_reading);
    mask: another mask than the spec's (the CPU tests)"""
    c, kind, canvas, fmt, order, swap = s["c"], s["kind"], s["canvas"], s["fmt"], s["order"], s["swap"]
    f1, f2, sw, sh = c["f1"], c["f2"], c["sw"], c["sh"]
    if wrong2:
        B = (to_rgba(orc, f2, c["frames2"][i], sw, sh, order ^ swap, c["L2"], is_422=0) if f2 == YUV422P else
             to_rgba(orc, f2, c["frames2"][i], sw, sh, order ^ swap, c["L2"], read_as=UYVY + YUYV - f2))
    else:
        B = to_rgba(orc, f2, c["frames2"][i], sw, sh, order ^ swap, c["L2"])
    A = to_rgba(orc, f1, c["frames"][i], sw, sh, order, c["L1"])
    if swap:
        sw_ = np.zeros((sh, sw * 4), np.uint8)
        orc.orc_swizzle(po.OPS.index("swap3postalpha"), 0, P(A), sw * 4, P(sw_), sw * 4, sw, sh, None)
        A = sw_
    w, h = sw, sh
    if canvas:
        A, B = letterboxed(orc, A, sw, sh, canvas), letterboxed(orc, B, sw, sh, canvas)
        w, h = canvas[0], canvas[1]
    m = mask if mask is not None else (s["masks"][i] if kind == DISSOLVE else None)
    out = select_oracle(orc, kind, A, B, w, h, s["amounts"][i], m)
    lut = s["lut"]
    if lut is not None:
        orc.orc_gamma_apply(P(out), w * 4, w, h, 4, 0, P(lut))
    if fmt == RGBA:
        return [out]
    want, _ = po.k4_out_planes(0, sw, sh, fmt, 0)
    wp, ws = po.planes_args(want)
    assert orc.orc_rgb_to_yuv(P(out), out.strides[0], sw, sh, order ^ swap, 1, ctypes.addressof(wp), ctypes.addressof(ws), fmt, 0, s["wt_sink"]) == 0
    return want


# ---- premises and the choice of amounts -------------------------------------------------------------------------------------------------------------------------------
def figure_of(sw, sh, canvas):
    """(figure width, figure height, the frame's origin on it)"""
    return (canvas[0], canvas[1], canvas[2], canvas[3]) if canvas else (sw, sh, 0, 0)


def premises(orc, kind, sw, sh, canvas, amount, mask, cross=None, first=True):
    """what a GPU case's selection map must show, as a dict of booleans (every one must be True).  both: the frame shows both layers; canvas: the map differs from the
    one computed on the frame's own size and origin; bars: an iris reaches into the bars; ps3: an iris's map differs from the one computed with 3-byte pixels (the
    circle on an even figure width: it is the SAME, see the module's docstring); cross = (axis, at): both layers on either side of a workgroup boundary.
    first: the case's first track.  `bars` and `ps3` are asked of that one only: a call of 64 tracks wants 64 amounts, and at 36x10 only eight of the 127 candidates
    put the rectangle's edge where the two pixel sizes round apart"""
    fw, fh, ox, oy = figure_of(sw, sh, canvas)
    whole = sel_map(orc, kind, fw, fh, amount, mask)
    m = whole[oy:oy + sh, ox:ox + sw]
    out = {"both": bool(m.any() and not m.all())}
    if canvas:
        own = sel_map(orc, kind, sw, sh, amount, mask[:sw * sh] if mask is not None else None)
        out["canvas"] = bool((m != own).any())
        if kind != DISSOLVE and first:
            outside = whole.copy()
            outside[oy:oy + sh, ox:ox + sw] = False
            out["bars"] = bool(outside.any())
    if kind != DISSOLVE and first:
        differs = bool((sel_map(orc, kind, fw, fh, amount, None, ps=3) != whole).any())
        out["ps3"] = differs if (kind == RECT or fw & 1) else not differs
    if cross:
        axis, at = cross
        a, b = (m[:, :at], m[:, at:]) if axis == "x" else (m[:at], m[at:])
        out["cross"] = all(bool(p.any() and not p.all()) for p in (a, b))
    return out


CANDIDATES = [int(k) / 128. for k in np.random.default_rng(0xA110).permutation(127) + 1]          # 1/128 .. 127/128 in one fixed shuffled order


def choose_amounts(orc, kind, sw, sh, canvas, masks, n, cross=None):
    """n distinct amounts strictly between 0 and 1, track t's the first unused candidate that holds every premise (with track t's mask)"""
    out, used = [], set()
    for t in range(n):
        for a in CANDIDATES:
            if a not in used and all(premises(orc, kind, sw, sh, canvas, a, masks[t] if masks else None, cross, first=t == 0).values()):
                used.add(a)
                out.append(a)
                break
        else:
            raise AssertionError("no amount holds the premises: kind %d, %dx%d on %s, track %d" % (kind, sw, sh, canvas, t))
    return out


def spec(orc, seed, pair, sw, sh, kind, fmt=RGBA, ntracks=2, canvas=None, amounts=None, ends=False, lut=None, order=0, swap=0, L1=None, L2=None, wt_sink=0, yvu_sink=False,
         pads=(8, 3, 5), dst_off=0, l1_offs=None, l2_offs=None, mask_odd=False, flat=None, cross=None):
    """one GPU case: the frames (tests/test_chain_flat_mix422.py's case(); flat = ((y, u, v), (y2, u2, v2)): constant YUV420P planes instead), the dissolve masks (one
    seed per track, canvas-sized on a canvas) and the amounts (chosen to hold the premises unless given; ends: the amounts are 0 and 1 and the map is single-layer)"""
    f1, f2 = pair
    seed = [int(v) for v in np.atleast_1d(seed)]
    c = case(seed, f1, f2, sw, sh, fmt, ntracks=ntracks, L1=L1, L2=L2, amounts=[0] * ntracks)
    if flat:
        def const(yuv):
            Y, U, V, st = flat_planes(sw, sh, *yuv)
            return ([Y, U, V], st)
        c["frames"], c["frames2"] = [const(flat[0])] * ntracks, [const(flat[1])] * ntracks
    fw, fh, _, _ = figure_of(sw, sh, canvas)
    base = int(np.random.default_rng(seed + [7]).integers(1 << 30))
    masks = [mask_of(orc, base + 977 * t, fw, fh) for t in range(ntracks)] if kind == DISSOLVE else None
    if amounts is None:
        amounts = choose_amounts(orc, kind, sw, sh, canvas, masks, ntracks, cross)
    assert len(amounts) == ntracks
    return dict(c=c, seed=seed, kind=kind, fmt=fmt, canvas=canvas, amounts=[float(a) for a in amounts], ends=ends, masks=masks, lut=lut, order=order, swap=swap, wt_sink=wt_sink,
                yvu_sink=yvu_sink, pads=pads, dst_off=dst_off, l1_offs=l1_offs, l2_offs=l2_offs, mask_odd=mask_odd, cross=cross)


def what(s):
    c = s["c"]
    return "%s, %s over %s, %dx%d%s, fmt %d" % (KIND_NAME[s["kind"]], NAME[c["f2"]], NAME[c["f1"]], c["sw"], c["sh"], " on %s" % (s["canvas"],) if s["canvas"] else "", s["fmt"])


# ---- the device's side -----------------------------------------------------------------------------------------------------------------------------------------------
def up_mask(m, odd=False):
    """a dissolve mask on the device; odd: at an address of 4 mod 8"""
    import torch
    t = torch.empty(m.size + 3, dtype=torch.float32, device="cuda")
    k = (int(odd) - (t.data_ptr() // 4)) % 2                  # skip one float where the tensor's own address has the other parity
    v = t[k:k + m.size]
    v.copy_(torch.from_numpy(m))
    assert v.data_ptr() % 8 == (4 if odd else 0)
    return v


def run(gpu, orc, s):
    """one call with tracks that all differ; the device buffers are allocated in a shuffled order and handed over in another (slot order != frame order); every
    destination plane is compared whole: frame bytes against the oracle, row padding and guard rows against their fill"""
    ops = gpu
    c, kind, canvas, fmt, order, swap = s["c"], s["kind"], s["canvas"], s["fmt"], s["order"], s["swap"]
    f1, f2, sw, sh, n = c["f1"], c["f2"], c["sw"], c["sh"], c["ntracks"]
    rng = np.random.default_rng(s["seed"] + [3])
    fw, fh, _, _ = figure_of(sw, sh, canvas)
    dims = plane_dims(fmt, fw, fh)
    pads = s["pads"]
    strides = [align(b + pads[k], 4 if fmt in (RGBA, UYVY, YUYV) else 2 if k == 0 else 1) for k, (b, _) in enumerate(dims)]
    fills = [[rng.integers(0, 256, (r + GUARD, strides[k]), dtype=np.uint8) for k, (_, r) in enumerate(dims)] for _ in range(n)]
    d1, d2, d_pl, dm = [None] * n, [None] * n, [None] * n, [None] * n
    l1_offs, l2_offs = s["l1_offs"], s["l2_offs"]
    for i in rng.permutation(n):
        d_pl[i] = [dev_at(f, s["dst_off"] if k == 0 else 0) for k, f in enumerate(fills[i])]
        if kind == DISSOLVE:
            dm[i] = up_mask(s["masks"][i], s["mask_odd"])
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
    ops.chain_flat_yuv_select(prm, src, src2, trk, kind, np.array([s["amounts"][k] for k in slots], np.float64), masks=[dm[k] for k in slots] if kind == DISSOLVE else None,
                              sink=sink, canvas=canvas)
    wants = []
    for i in range(n):
        want = expected_select(orc, s, i)
        wants.append(want)
        for p, j in enumerate(dsel):              # p: the conversion's plane (Y, U, V); j: the buffer it was handed
            b, r = dims[p]
            got = host(d_pl[i][j])
            bad = got[:r, :b] != want[p][:r, :b]
            assert not bad.any(), "%s, track %d (amount %s) plane %d: %d bytes differ from the oracle, first at %s" % (
                what(s), i, s["amounts"][i], p, int(bad.sum()), np.argwhere(bad)[0].tolist())
            assert (got[:r, b:] == fills[i][j][:r, b:]).all(), "%s, track %d plane %d: row padding was written" % (what(s), i, p)
            assert (got[r:] == fills[i][j][r:]).all(), "%s, track %d plane %d: guard rows were written" % (what(s), i, p)
    return wants


# ---- the case lists: generators of specs, walked by the GPU tests and by the CPU test of their premises ----------------------------------------------------------------
def pair_layers(pair, j):
    """the j-th variation of how the two layers are laid out and converted: tables (0 / 1 for a packed layer), quality LOW .. HIGH, LGPU_YUV_FIX_EDGES, pitches, tight
    chroma planes, plane order -- varied across the cases, not multiplied out"""
    f1, f2 = pair
    wt1 = (j & 1) if packed(f1) else j & 3
    wt2 = ((j >> 1) & 1) if packed(f2) else (j + 1 + (j >> 2)) & 3
    return (layer(wt=wt1, q=1 + j % 3, fix=j & 1, pad=(4 * (j & 1), 1, 3), tight=bool(j & 2), yvu=bool(j & 4)),
            layer(wt=wt2, q=3 - j % 3, fix=1 - (j & 1), pad=(4 - 4 * (j & 1), 3, 1), tight=not j & 2, yvu=not j & 4))


def stage_specs(orc, pair):
    """test 4: 3 kinds x {RGBA, packed, YUV420P} sinks at 34x7 (no trailing row) and 36x6 (one; the 4:2:0 sink takes the even height only); a packed format is UYVY on
    the first size and YUYV on the second.  LUT, swap_rb, out_order, table sets, pb_quality, FIX_EDGES and the sink's tables and plane order move on with every case"""
    j = ALL_PAIRS.index(pair)
    for kind in KINDS:
        for fmt in (RGBA, UYVY, YUV420P):
            for i, (sw, sh) in enumerate([(34, 7), (36, 6)]):
                if fmt == YUV420P and sh & 1:
                    continue
                j += 1
                f1, f2 = (YUYV if i and f == UYVY else f for f in pair)
                L1, L2 = pair_layers((f1, f2), j)
                out = YUYV if (fmt == UYVY and i) else fmt
                yield spec(orc, [0x5E1, ALL_PAIRS.index(pair), kind, fmt, i], (f1, f2), sw, sh, kind, out, ntracks=2, L1=L1, L2=L2, lut=[None, "gamma", INVERTED][j % 3],
                           order=(j >> 1) & 1, swap=j & 1, wt_sink=(j % 4) if fmt == YUV420P else j & 1, yvu_sink=bool(j & 2), pads=(8 * (j & 1), 3, 5))


def small_specs(orc, sw, sh):
    """test 5: every kind on the walks' smallest frames, to RGBA and (even heights) to YUV420P"""
    for p, pair in enumerate(SMALL_PAIRS):
        for kind in KINDS:
            for fmt in (RGBA, YUV420P):
                if fmt == YUV420P and sh & 1:
                    continue
                j = p + kind + fmt
                L1, L2 = pair_layers(pair, j)
                yield spec(orc, [0x5E2, sw, sh, p, kind, fmt], pair, sw, sh, kind, fmt, ntracks=2, L1=L1, L2=L2, lut="gamma" if j & 1 else None, swap=j & 1, order=(j >> 1) & 1,
                           wt_sink=j & 1, pads=(2, 1, 3) if fmt == YUV420P else (8, 3, 5))


def wide_tall_specs(orc, kind):
    """test 6: 1030 pixels: 515 cells per row, three workgroups along x with the last one partly empty, the figure across the boundary at x = 512; a frame of width 16
    with more units than a launch has workgroup rows, so a workgroup walks a run of units, the figure across a boundary between two runs in the middle"""
    tall = 2 * UNIT_CAP + 6
    per = -(-(tall // 2 + 1) // UNIT_CAP)                     # units per workgroup (flat_select.hip: ceil(nunits / cap))
    assert per == 2
    mid = (tall // 4 // per) * per                            # a run starts at this unit, near the middle: its first row is 2 * mid - 1
    for t, (pair, fmt) in enumerate([((UYVY, YUV422P), RGBA), ((YUV420P, YUYV), YUV420P)]):
        yield spec(orc, [0x5E3, kind, t, 0], pair, 1030, 6 if fmt == YUV420P else 5, kind, fmt, ntracks=1, L1=layer(tight=True, pad=(0, 1, 1)), L2=layer(fix=1, pad=(4, 0, 3), tight=True),
                   lut="gamma", cross=("x", 512))
        yield spec(orc, [0x5E3, kind, t, 1], pair, 16, tall, kind, fmt, ntracks=1, L1=layer(fix=1, pad=(4, 1, 1)), L2=layer(wt=1, pad=(0, 1, 0), tight=True), swap=1,
                   cross=("y", 2 * mid - 1))


SWEEP_33 = [k / 32. for k in range(33)]
# 64 amounts, both ends among them: the 33 above and the odd 64ths from 3/64 on (at 1/64 the rectangle of a 66x34 frame is empty, which only an end may be)
SWEEP_64 = SWEEP_33 + [(2 * k + 1) / 64. for k in range(1, 32)]


def sweep_specs(orc, kind):
    """test 7: constant black on layer 1 and constant white on layer 2, so the output IS the selection map: the uthr bisection, the byte insets, the 33-track split"""
    for amounts in (SWEEP_33, SWEEP_64):
        yield spec(orc, [0x5E4, kind, len(amounts)], (YUV420P, YUV420P), 66, 34, kind, RGBA, ntracks=len(amounts), amounts=amounts, ends=True, flat=((16, 128, 128), (235, 128, 128)))


CANVASES = [(34, 7, (40, 12, 3, 2)), (34, 7, (40, 12, 3, 3)), (34, 8, (34, 12, 0, 2)), (34, 7, (41, 12, 4, 2))]          # the second and third are centred; the last is of odd width


def canvas_specs(orc, kind):
    """test 8: the figure is the canvas's and crosses the frame's edges into the bars; the dissolve mask is canvas-sized; under a LUT the bars are LUT(black)"""
    for k, (sw, sh, cv) in enumerate(CANVASES):
        assert ((cv[2], cv[3]) == ((cv[0] - sw + 1) >> 1, (cv[1] - sh + 1) >> 1)) == (k in (1, 2))
        pair = ALL_PAIRS[(3 * kind + 2 * k) % len(ALL_PAIRS)]
        L1, L2 = pair_layers(pair, k + kind)
        yield spec(orc, [0x5E5, kind, k], pair, sw, sh, kind, RGBA, ntracks=2, canvas=cv, L1=L1, L2=L2, lut=[INVERTED, "gamma", None, INVERTED][k], swap=k & 1, order=(k >> 1) & 1,
                   pads=(4 * k, 0, 0))


def track_specs(orc, ntracks):
    """test 9: distinct amounts, masks and frames on every track; 32 tracks per launch, so 33 and 64 go as two"""
    for kind, fmt, pair in ((RECT, RGBA, (UYVY, YUV422P)), (CIRCLE, YUV420P, (YUV420P, UYVY)), (DISSOLVE, UYVY, (YUV422P, YUV420P))):
        yield spec(orc, [0x5E6, ntracks, kind], pair, 36, 10, kind, fmt, ntracks=ntracks, L1=layer(wt=1, pad=(4, 1, 3)), L2=layer(wt=0 if packed(pair[1]) else 2, pad=(0, 3, 1)),
                   lut="gamma", swap=ntracks & 1, wt_sink=int(fmt == YUV420P) * 2, yvu_sink=True)


def address_specs(orc, dst_off):
    """test 10: the destination at 4 and 12 mod 16 with pitches of 4 mod 8 (4-byte stores where the address is no multiple of 8), the 4:2:0 luma plane at 2 mod 4; packed
    layers at 0, 4, 8 and 12 mod 16; planar layers' planes at odd addresses with odd pitches, as the mix form allows; the dissolve masks at 4 mod 8"""
    assert (132 * 4 + 4) % 8 == 4 and (132 * 2 + 4) % 8 == 4
    for n, off in enumerate((0, 4, 8, 12)):
        pair = [(YUV420P, UYVY), (YUV422P, YUYV), (YUYV, UYVY), (UYVY, YUYV)][n]
        l1_offs = (12 - off, 0, 0) if packed(pair[0]) else (1, 3, 5)
        for fmt, pads, doff in ((RGBA, (4, 0, 0), dst_off), (UYVY, (4, 0, 0), dst_off), (YUV420P, (2, 1, 1), dst_off + 2)):
            yield spec(orc, [0x5E7, dst_off, off, fmt], pair, 132, 8, KINDS[(n + fmt) % 3], fmt, ntracks=2, L1=layer(pad=(4, 1, 1)), L2=layer(pad=(4 * (n & 1), 0, 0), wt=1), pads=pads,
                       dst_off=doff, l1_offs=l1_offs, l2_offs=(off, 0, 0), mask_odd=True, lut="gamma" if fmt == RGBA else None)
    for k, (pair, offs) in enumerate((((UYVY, YUV422P), (1, 3, 5)), ((YUV422P, YUV420P), (3, 1, 7)), ((YUV420P, YUV422P), (5, 7, 1)))):
        for fmt, pads, doff in ((RGBA, (4, 0, 0), dst_off), (YUV420P, (2, 1, 1), dst_off + 2)):
            yield spec(orc, [0x5E7, dst_off, k, fmt, 1], pair, 132, 8, KINDS[k], fmt, ntracks=2, L2=layer(pad=(1, 3, 1), wt=1), pads=pads, dst_off=doff, l2_offs=offs, mask_odd=bool(fmt))


# the figures of the cases at 1920x1080 (tests 11 and 12 draw their frames on the device): (kind, amount, mask seed); an end is amount 0 or 1
# the rectangle's amount puts its left edge where 4-byte and 3-byte pixels round apart: 960 * (1 - 0.3707) = 604.13, and the fractions in [1/8, 1/6) do that
AT_SIZE = [(RECT, 0.3707, 0), (CIRCLE, 0.61, 0), (DISSOLVE, 0.45, 0xD155)]
ENDS = [(kind, a, 0xE2D5) for kind in KINDS for a in (0., 1.) if (kind, a) != (CIRCLE, 0.)]          # the circle at amount 0 shows its centre pixel from layer 2: no end


def with_lut(orc, s):
    """the spec with its LUT in place: "gamma" is tests/test_chain_flat.py's gamma_lut"""
    return dict(s, lut=gamma_lut(orc) if isinstance(s["lut"], str) else s["lut"])


def all_spec_lists(orc):
    """every generator above with every parameter its GPU test runs it with: (name, generator)"""
    for pair in ALL_PAIRS:
        yield "stages " + pair_id(pair), stage_specs(orc, pair)
    for sw, sh in SMALL:
        yield "small %dx%d" % (sw, sh), small_specs(orc, sw, sh)
    for kind in KINDS:
        yield "wide and tall " + KIND_NAME[kind], wide_tall_specs(orc, kind)
        yield "sweep " + KIND_NAME[kind], sweep_specs(orc, kind)
        yield "canvas " + KIND_NAME[kind], canvas_specs(orc, kind)
    for n in (1, 16, 33, 64):
        yield "tracks %d" % n, track_specs(orc, n)
    for off in (4, 12):
        yield "addresses %d" % off, address_specs(orc, off)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_select_symbol_struct_and_wrapper():
    """1. the entry point is in the built library under a prototype of its own, lgpu_select is laid out as include/lives_gpu_select.h has it (int, two pointers: 24
    bytes on LP64), the wrapper fills it, and the header is not lives_gpu.h: that one declares nothing of this form"""
    import os
    import re
    from lives_amd import lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "lives_gpu_select.h")).read(), flags=re.S)
    assert re.findall(r"\b(lgpu_[a-z0-9_]+)\s*\(", text) == ["lgpu_chain_flat_yuv_select"] and '#include "lives_gpu.h"' in text
    m = re.search(r"typedef struct \{\s*int kind;\s*const double \*amounts;\s*const float \*const \*mask_d;\s*\} lgpu_select;", text)
    assert m, "lgpu_select is not laid out as the ctypes struct reads it"
    assert "lgpu_chain_flat_yuv_select" not in open(os.path.join(root, "include", "lives_gpu.h")).read()
    assert "lgpu_chain_flat_yuv_select" not in lib.PROTOTYPES and len(lib.SELECT_PROTOTYPES["lgpu_chain_flat_yuv_select"]) == 9
    S = lib.Select
    assert ctypes.sizeof(S) == 24 and S.kind.offset == 0 and S.amounts.offset == 8 and S.mask_d.offset == 16
    L = lib.load()
    assert hasattr(L, "lgpu_chain_flat_yuv_select") and L.lgpu_chain_flat_yuv_select.argtypes == lib.SELECT_PROTOTYPES["lgpu_chain_flat_yuv_select"]
    assert (lib.SELECT_IRIS_RECT, lib.SELECT_IRIS_CIRCLE, lib.SELECT_DISSOLVE, lib.LGPU_CHAIN_SELECT_TRACKS) == (0, 1, 3, 32)
    s = ops.select(3, [0.25, 1.0], masks=[0x1000, 0x2000])
    assert (s.kind, s.amounts[0], s.amounts[1], s.mask_d[0], s.mask_d[1]) == (3, 0.25, 1.0, 0x1000, 0x2000)
    s = ops.select(1, [0.5])
    assert s.kind == 1 and s.amounts[0] == 0.5 and not s.mask_d
    assert callable(ops.chain_flat_yuv_select)


def test_every_gpu_case_holds_its_premises(orc):
    """2. for every GPU case and every track of it: the selection map shows both layers -- unless the case is named as an end, and then only at amounts 0 and 1, where it
    is single-layer; on a canvas the map differs from the one of the frame's own size and origin and the first track's iris reaches into the bars; the first track's
    iris map differs from the 3-byte one (the circle on an even width: equals it); the wide and tall cases have both layers on either side of their workgroup boundary"""
    ncases = 0
    for name, gen in all_spec_lists(orc):
        for s in gen:
            c = s["c"]
            for t, a in enumerate(s["amounts"]):
                mask = s["masks"][t] if s["masks"] else None
                if s["ends"] and a in (0., 1.):
                    fw, fh, ox, oy = figure_of(c["sw"], c["sh"], s["canvas"])
                    m = sel_map(orc, s["kind"], fw, fh, a, mask)[oy:oy + c["sh"], ox:ox + c["sw"]]
                    if s["kind"] == CIRCLE and a == 0.:          # the centre pixel alone (the module's docstring)
                        assert m.sum() == 1 and m[fh >> 1, fw >> 1], "%s: %s track %d: the circle at amount 0 shows more than its centre" % (name, what(s), t)
                    else:
                        assert (m == bool(a)).all(), "%s: %s track %d: amount %s is not single-layer" % (name, what(s), t, a)
                    continue
                assert 0. < a < 1.
                pr = premises(orc, s["kind"], c["sw"], c["sh"], s["canvas"], a, mask, s["cross"], first=t == 0)
                if s["ends"]:
                    pr = {"both": pr["both"]}          # the figure sweep: its amounts are given, and between the ends they must still show both layers
                assert all(pr.values()), "%s: %s track %d, amount %s: %s" % (name, what(s), t, a, pr)
            ncases += 1
    assert ncases > 250
    # the frames at 1920x1080, and the two ends
    for kind, a, seed in AT_SIZE:
        mask = mask_of(orc, seed, 1920, 1080) if kind == DISSOLVE else None
        assert all(premises(orc, kind, 1920, 1080, None, a, mask).values()), (kind, a)
    for kind, a, seed in ENDS:
        m = sel_map(orc, kind, 1920, 1080, a, mask_of(orc, seed, 1920, 1080) if kind == DISSOLVE else None)
        assert (m == bool(a)).all(), (kind, a)
    # an even figure width: the circle's map is the same at either pixel size, whatever the amount (why `ps3` asks for equality there)
    for a in CANDIDATES[:16]:
        assert (sel_map(orc, CIRCLE, 34, 7, a, None, ps=3) == sel_map(orc, CIRCLE, 34, 7, a, None)).all()


@pytest.mark.parametrize("pair", [p for p in ALL_PAIRS if p[1] != YUV420P], ids=pair_id)
def test_expectation_tells_layer2s_format_and_the_mask(orc, pair):
    """3. on the frames test_select_stages draws: reading layer 2 as the wrong format changes every track's expectation (YUV422P as 4:2:0, UYVY as YUYV and the
    reverse), and so does the mask of another seed in the dissolve cases"""
    n = 0
    for s in stage_specs(orc, pair):
        s = with_lut(orc, s)
        c = s["c"]
        fw, fh, _, _ = figure_of(c["sw"], c["sh"], s["canvas"])
        for i in range(c["ntracks"]):
            right = expected_select(orc, s, i)
            assert any((a != b).any() for a, b in zip(right, expected_select(orc, s, i, wrong2=True))), "%s: layer 2 read wrongly gives the same bytes" % what(s)
            if s["kind"] == DISSOLVE:
                assert any((a != b).any() for a, b in zip(right, expected_select(orc, s, i, mask=mask_of(orc, 0xBAD5EED + i, fw, fh)))), "%s: another mask gives the same bytes" % what(s)
                n += 1
    assert n >= 6


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------------------
def go(gpu, orc, specs):
    n = 0
    for s in specs:
        run(gpu, orc, with_lut(orc, s))
        n += 1
    assert n


# The GPU tests walk their lists in one test each, not one test per parameter: a case is a call of a few milliseconds, every assertion names its case (what()), and the
# whole file runs in about two seconds.
@pytest.mark.gpu
def test_select_stages(gpu, orc):
    """4. every kind to every destination, all nine format pairs with UYVY as the packed format plus two YUYV pairs (stage_specs)"""
    for pair in ALL_PAIRS:
        go(gpu, orc, stage_specs(orc, pair))


@pytest.mark.gpu
def test_select_frame_shapes(gpu, orc):
    """5. the smallest frames: row 0 alone, with and without a row pair and the trailing row, one and three cells wide (small_specs).
    6. wide and tall: three workgroups across a row, the last partial; a workgroup that walks a run of units; the figure across a workgroup boundary in both
    (wide_tall_specs)"""
    for sw, sh in SMALL:
        go(gpu, orc, small_specs(orc, sw, sh))
    for kind in KINDS:
        go(gpu, orc, wide_tall_specs(orc, kind))


@pytest.mark.gpu
def test_select_figures(gpu, orc):
    """7. the figure sweep: per kind one call of 33 tracks, then one of 64, at 66x34 over constant black and constant white: the output is the selection map at amounts
    from 0 to 1 (sweep_specs).
    8. the canvas: 34x7 on 40x12 at (3, 2) and centred, 34x8 on 34x12 (bars above and below only), 34x7 on a canvas of odd width (canvas_specs)"""
    for kind in KINDS:
        go(gpu, orc, sweep_specs(orc, kind))
        go(gpu, orc, canvas_specs(orc, kind))


@pytest.mark.gpu
def test_select_tracks_and_addresses(gpu, orc):
    """9. 1, 16, 33 and 64 tracks with distinct amounts, masks and frames in shuffled buffers (track_specs).
    10. each alignment class the entry point and the kernel tell apart (address_specs)"""
    for ntracks in (1, 16, 33, 64):
        go(gpu, orc, track_specs(orc, ntracks))
    for dst_off in (4, 12):
        go(gpu, orc, address_specs(orc, dst_off))


def clips(w, h, n, f1, f2, seed):
    """n frames per layer drawn on the device: ((planes per format, strides), (..))"""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)

    def clip(f):
        rnd = lambda r, b: [torch.randint(0, 256, (r, b), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
        if packed(f):
            return [rnd(h, w * 2), None, None], (w * 2,)
        ch = h // 2 if f == YUV420P else h
        return [rnd(h, w), rnd(ch, w // 2), rnd(ch, w // 2)], (w, w // 2, w // 2)
    return clip(f1), clip(f2)


def plane_size(pl, k):
    return 0 if pl[k] is None else pl[k][0].numel()


def ends_are_the_single_layer_forms(gpu, orc, fmt):
    """11. 2 x 1920x1080, UYVY over YUV420P: at amount 0 every kind (but the circle, whose centre pixel is layer 2's there) gives the bytes of layer 1's single-layer flat form (lgpu_chain_flat_yuv420p[_to_yuv] with
    LGPU_INTERP_NOBLEND), at amount 1 those of layer 2's (lgpu_chain_flat_yuv422 on layer 2's frames, no R <-> B: src2->out_order is the chain's order already)"""
    import torch
    ops = gpu
    w, h, n = 1920, 1080, 2
    f1, f2 = YUV420P, UYVY
    (A, st1), (B, st2) = clips(w, h, n, f1, f2, 0xE2D + fmt)
    lut = gamma_lut(orc)
    dims = plane_dims(fmt, w, h)
    new = lambda fill: [[torch.full((r, b), fill, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
    sink = ops.chain_sink(fmt, [b for (b, _) in dims], which_tables=0, in_order=1) if fmt != RGBA else None
    prm = ops.chain_params(w, h, 0, w, h, 0, w * 4, swap_rb=1, interp=PIXBUF, bf=0, lut=lut)
    s1 = ops.yuv_layer_source(f1, st1, plane_size(A, 1), plane_size(A, 2), out_order=0, which_tables=1, pb_quality=2)
    s2 = ops.yuv_layer_source(f2, st2, 0, 0, out_order=1, which_tables=0, pb_quality=2)
    # layer 1 alone: [R <-> B] and the LUT ride in the flat form; layer 2 alone: converted in the chain's order, so no swap
    alone = [new(0xC5), new(0xC5)]
    flat = ops.chain_params(w, h, 0, w, h, 0, w * 4, swap_rb=1, interp=PIXBUF | NOBLEND, bf=0, lut=lut)
    src1 = ops.yuv_source(st1, plane_size(A, 1), plane_size(A, 2), out_order=0, which_tables=1, pb_quality=2)
    if fmt == RGBA:
        ops.chain_flat_yuv420p(flat, src1, ops.chain_yuv_tracks(A[0], A[1], A[2], None, [t[0] for t in alone[0]]), None)
    else:
        ops.chain_flat_yuv420p_to_yuv(flat, src1, sink, ops.chain_yuv_sink_tracks(A[0], A[1], A[2], None, alone[0]), None)
    flat2 = ops.chain_params(w, h, 0, w, h, 0, w * 4, swap_rb=0, interp=PIXBUF | NOBLEND, bf=0, lut=lut)
    ops.chain_flat_yuv422(flat2, ops.yuv422_source(f2, st2, 0, 0, out_order=1, which_tables=0, pb_quality=2), ops.chain_yuv_sink_tracks(B[0], None, None, None, alone[1]), None, sink=sink)
    masks = [torch.from_numpy(mask_of(orc, ENDS[0][2] + t, w, h)).cuda() for t in range(n)]
    for kind, amount, _ in ENDS:
        out = new(0x5C)
        ops.chain_flat_yuv_select(prm, s1, s2, ops.chain_yuv_mix_tracks(A[0], A[1], A[2], B[0], None, None, out), kind, [amount] * n, masks=masks if kind == DISSOLVE else None, sink=sink)
        torch.cuda.synchronize()
        for t in range(n):
            for p in range(len(dims)):
                assert torch.equal(out[t][p], alone[int(amount)][t][p]), "%s at amount %s, track %d plane %d: %d bytes differ from layer %d's single-layer form" % (
                    KIND_NAME[kind], amount, t, p, int((out[t][p] != alone[int(amount)][t][p]).sum()), 1 + int(amount))
    assert not torch.equal(alone[0][0][0], alone[1][0][0])


def at_size_matches_todays_launches(gpu, orc, k):
    """12. 2 x 1920x1080, one case per kind: byte-identical to the device's own launches on the same inputs -- the two conversions, lgpu_swizzle, lgpu_transition /
    lgpu_dissolve, lgpu_gamma_apply [, lgpu_rgb_to_yuv]: the rectangle UYVY over YUV420P to RGBA, the circle YUV422P over YUV422P to UYVY, the dissolve YUV420P over
    UYVY to YUV420P"""
    import torch
    from lives_amd import lib
    ops = gpu
    kind, amount, seed = AT_SIZE[k]
    (f1, f2), fmt = [((YUV420P, UYVY), RGBA), ((YUV422P, YUV422P), UYVY), ((UYVY, YUV420P), YUV420P)][k]
    w, h, n = 1920, 1080, 2
    (A, st1), (B, st2) = clips(w, h, n, f1, f2, 0xA75 + k)
    lut = gamma_lut(orc)
    dims = plane_dims(fmt, w, h)
    fused = [[torch.full((r, b), 0x5C, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
    today = [[torch.full((r, b), 0xC5, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
    sink = ops.chain_sink(fmt, [b for (b, _) in dims], which_tables=0, in_order=1) if fmt != RGBA else None
    prm = ops.chain_params(w, h, 0, w, h, 0, w * 4, swap_rb=1, interp=PIXBUF, bf=0, lut=lut)
    wt1, wt2 = 0, 0 if packed(f1) or packed(f2) else 1
    s1 = ops.yuv_layer_source(f1, st1, plane_size(A, 1), plane_size(A, 2), out_order=0, which_tables=wt1, pb_quality=2)
    s2 = ops.yuv_layer_source(f2, st2, plane_size(B, 1), plane_size(B, 2), out_order=1, which_tables=wt2, pb_quality=3, flags=1 if f2 == YUV420P else 0)
    masks = [torch.from_numpy(mask_of(orc, seed + t, w, h)).cuda() for t in range(n)] if kind == DISSOLVE else None
    ops.chain_flat_yuv_select(prm, s1, s2, ops.chain_yuv_mix_tracks(A[0], A[1], A[2], B[0], B[1], B[2], fused), kind, [amount] * n, masks=masks, sink=sink)

    def convert(f, pl, t, dst, order, wt, q, flags):
        if packed(f):
            ops.yuv_to_rgb([pl[0][t]], dst, w, h, f, 0, order, 1, wt)
        else:
            ops.yuv420p_to_rgb(pl[0][t], pl[1][t], pl[2][t], dst, w, h, 4, order, int(f == YUV422P), wt, q, flags=flags)
    for t in range(n):
        a, a2, b = (torch.zeros((h, w * 4), dtype=torch.uint8, device="cuda") for _ in range(3))
        convert(f2, B, t, b, 1, wt2, 3, 1 if f2 == YUV420P else 0)
        convert(f1, A, t, a, 0, wt1, 2, 0)
        ops.swizzle(lib.SWAP3POSTALPHA, a, a2, w, h)
        res = today[t][0] if fmt == RGBA else torch.zeros((h, w * 4), dtype=torch.uint8, device="cuda")
        if kind == DISSOLVE:
            ops.dissolve(a2, b, res, w, h, 4, masks[t], amount)
        else:
            ops.transition(kind, a2, b, res, w, h, 4, amount)
        ops.gamma_apply(res, w, h, 4, lut)
        if fmt != RGBA:
            ops.rgb_to_yuv(res, today[t], w, h, 1, 1, fmt, 0, 0)
    torch.cuda.synchronize()
    for t in range(n):
        for p in range(len(dims)):
            assert torch.equal(fused[t][p], today[t][p]), "track %d plane %d: %d bytes differ from today's launches" % (t, p, int((fused[t][p] != today[t][p]).sum()))
    assert not bool((fused[0][0] == 0x5C).all())


@pytest.mark.gpu
def test_select_at_1920x1080(gpu, orc):
    """11. the ends, device against device, to RGBA and to UYVY (ends_are_the_single_layer_forms).  12. one case per kind against today's launches
    (at_size_matches_todays_launches)"""
    for fmt in (RGBA, UYVY):
        ends_are_the_single_layer_forms(gpu, orc, fmt)
    for k in range(len(AT_SIZE)):
        at_size_matches_todays_launches(gpu, orc, k)


@pytest.mark.gpu
def test_select_refusals(gpu):
    """13. the refusals, for three format pairs (refusals_of)"""
    for pair in ((YUV422P, UYVY), (YUYV, YUV420P), (YUV420P, YUV422P)):
        refusals_of(gpu, pair)


def refusals_of(gpu, pair):
    """13. every LGPU_E_BADARG and LGPU_E_UNSUPPORTED item of the entry point, one call each: the code is compared and the destinations' fill is still whole afterwards;
    the same call inside the form then runs"""
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
    M = torch.rand(CW * CH + 2, dtype=torch.float32, device="cuda")
    csize = lambda pl: 0 if pl[1] is None else pl[1].numel()
    ptr = lambda t: None if t is None else t.data_ptr()

    def call(fmt=RGBA, canvas=None, kind=RECT, amounts=(0.5,), masks="own", no_sel=False, sw_=w, sh_=h, dw_=None, dh_=None, interp=PIXBUF, blur=0, ntracks=1, null=None, strides=full1,
             strides2=full2, usz=None, usz2=None, order=0, order2=None, swap=0, wt_src=0, wt_src2=0, q=2, q2=2, flags2=0, wt=0, in_order=None, orow=None, dst_off=0, in_place=None,
             in_fmt=f1, in_fmt2=f2, off2=0, no_src2=False, mask_off=0):
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
        if masks == "own":
            masks = [M.data_ptr() + mask_off] * m
        am = list(amounts) * m if amounts is not None else None
        if no_sel or no_src2:
            sel = ops.select(kind, am, masks)
            cv = lib.Canvas(*canvas) if canvas else None
            return lib.load().lgpu_chain_flat_yuv_select(ctypes.byref(prm), ctypes.byref(src), None if no_src2 else ctypes.byref(src2), None if no_sel else ctypes.byref(sel),
                                                         ctypes.byref(cv) if cv else None, ctypes.byref(sink) if sink else None, trk, len(trk), ops.stream_ptr())
        return ops.chain_flat_yuv_select(prm, src, src2, trk, kind, am, masks=masks, sink=sink, canvas=canvas, check=False)

    cv0 = (CW, CH, 5, 3)
    badarg = {
        "kind 2 (4 way split)": dict(kind=2),
        "kind 4": dict(kind=4),
        "kind -1": dict(kind=-1),
        "null select": dict(no_sel=True),
        "null amounts": dict(amounts=None),
        "amount below 0": dict(amounts=(-0.01,)),
        "amount above 1": dict(amounts=(1.01,)),
        "amount NaN": dict(amounts=(float("nan"),)),
        "amount infinite": dict(amounts=(float("inf"),)),
        "dissolve without a mask table": dict(kind=DISSOLVE, masks=None),
        "dissolve with a null mask": dict(kind=DISSOLVE, masks=[None]),
        "dissolve mask at 2 mod 4": dict(kind=DISSOLVE, mask_off=2),
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
            rc = call(**kw)
            torch.cuda.synchronize()
            assert rc == want, "%s (%s): %d, expected %d (%s)" % (name, kw, rc, want, lib.load().lgpu_last_error())
            assert all(bool((d == 0x5C).all()) for d in D), "%s: a destination was written" % name
    # ... and the same call inside the form runs: every kind, to RGBA, onto the canvas and to both sinks; params->bf and LGPU_INTERP_NOBLEND are ignored
    for kind in KINDS:
        assert call(kind=kind) == 0 and call(kind=kind, canvas=cv0) == 0 and call(kind=kind, interp=PIXBUF | NOBLEND) == 0
        torch.cuda.synchronize()
        assert bool((D[0][:CH, 3:CW * 4:4] == 255).all()) and bool((D[0][CH:] == 0x5C).all()) and bool((D[0][:, CW * 4:] == 0x5C).all())          # every pixel's alpha
        assert call(kind=kind, fmt=UYVY) == 0 and call(kind=kind, fmt=YUV420P, amounts=(0.,)) == 0 and call(kind=kind, amounts=(1.,)) == 0
        torch.cuda.synchronize()
