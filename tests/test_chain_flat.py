"""lgpu_chain_flat_yuv420p / lgpu_chain_flat_yuv420p_to_yuv: the UNSCALED tick from decoded planar 4:2:0 frames as one launch (K2's conversion -> [R <-> B] ->
[letterbox] -> [chroma blend] -> [gamma LUT] -> RGBA, or -> K4's conversion to UYVY / YUYV / YUV420P; no RGBA frame in between) against the oracle's composition
orc_yuv420p_to_rgb -> [orc_swizzle] -> [orc_letterbox onto opaque black] -> [orc_blend_chroma] -> [orc_gamma_apply] -> [orc_rgb_to_yuv]; at size against the device's own
launches lgpu_yuv420p_to_rgb_batch + lgpu_chain_amounts + lgpu_rgb_to_yuv_batch; and the refusals.  Bit-exact: every byte of every destination plane, and every byte of
the planes' row padding and guard rows."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.chain_ref import BLACK, Tracks, distinct_amounts, planes
from tests.offset_buffers import dev_at
from tests.util import align, dev, host

P = po.P
PIXBUF, NOBLEND = 0x100, 0x400
E_BADARG, E_UNSUPPORTED = -2, -3
RGBA, UYVY, YUYV, YUV420P = 0, 2, 3, 4
FIX_EDGES = 1
GUARD = 2
UNIT_CAP = 2048          # flat.hip kFlatWgTarget: a launch of one track at width <= 512 walks at most this many units as one workgroup row each


def gamma_lut(orc):
    lut = np.zeros(256, np.uint8)
    assert orc.orc_gamma_lut8(1.0, po.GAMMA_SRGB, po.GAMMA_LINEAR, 1.4, P(lut)) == 1
    return lut


def planes_any(rng, sw, sh, pad, tight):
    """chain_ref.planes() for any height: (sh + 1) / 2 chroma rows (an odd height's last row has a chroma row of its own, as K2 reads it)"""
    Y, U, V, st = planes(rng, sw, (sh + 1) & ~1, pad, tight)
    return np.ascontiguousarray(Y[:sh]), U, V, st


def flat_planes(sw, sh, y, u, v):
    """a frame of one colour"""
    hw, hh = sw // 2, (sh + 1) // 2
    return (np.full((sh, sw), y, np.uint8), np.full(hh * hw, u, np.uint8), np.full(hh * hw, v, np.uint8), (sw, hw, hw))


def plane_dims(fmt, w, h):
    """(bytes per row, rows) of the destination's planes"""
    if fmt == RGBA:
        return [(w * 4, h)]
    return [(w * 2, h)] if fmt in (UYVY, YUYV) else [(w, h), (w >> 1, h >> 1), (w >> 1, h >> 1)]


def oracle_flat(orc, Y, U, V, strides, sw, sh, order, swap, wt, q, fix, l2, amount, lut, canvas=None, fmt=RGBA, wt_sink=0):
    """the no-scale sibling of chain_ref.oracle_chain: the list of destination planes one track must equal.  canvas = (nwidth, nheight, offs_x, offs_y)"""
    rgba = np.zeros((sh, sw * 4), np.uint8)
    st = (ctypes.c_int * 3)(*strides)
    orc.orc_yuv420p_to_rgb(P(Y), P(U), P(V), st, U.size, V.size, P(rgba), sw * 4, sw, sh, 4, order, 0, wt, q, None, fix)
    out = rgba
    if swap:
        out = np.zeros((sh, sw * 4), np.uint8)
        orc.orc_swizzle(po.OPS.index("swap3postalpha"), 0, P(rgba), sw * 4, P(out), sw * 4, sw, sh, None)
    w, h = sw, sh
    if canvas:
        w, h, ox, oy = canvas
        big = np.zeros((h, w * 4), np.uint8)
        if (ox, oy) == ((w - sw + 1) >> 1, (h - sh + 1) >> 1):          # where letterbox_layer centres the frame
            orc.orc_letterbox(P(out), sw * 4, sw, sh, P(big), w * 4, w, h, 4, P(BLACK))
        else:
            big[:, 3::4] = 255
            big[oy:oy + sh, ox * 4:(ox + sw) * 4] = out
        out = big
    if l2 is not None:
        orc.orc_blend_chroma(P(out), w * 4, P(l2), l2.strides[0], P(out), w * 4, w, h, 4, 0, amount)
    if lut is not None:
        orc.orc_gamma_apply(P(out), w * 4, w, h, 4, 0, P(lut))
    if fmt == RGBA:
        return [out]
    want, _ = po.k4_out_planes(0, sw, sh, fmt, 0)
    wp, ws = po.planes_args(want)
    assert orc.orc_rgb_to_yuv(P(out), out.strides[0], sw, sh, order ^ swap, 1, ctypes.addressof(wp), ctypes.addressof(ws), fmt, 0, wt_sink) == 0
    return want


def expected(orc, src, sw, sh, order, swap, wt_src, q, fix, yvu_src, l2, amount, lut, canvas, fmt, wt_sink):
    Y, A1, A2, (ys_, s1, s2) = src
    U, V, stri = (A2, A1, (ys_, s2, s1)) if yvu_src else (A1, A2, (ys_, s1, s2))
    return oracle_flat(orc, Y, U, V, stri, sw, sh, order, swap, wt_src, q, fix, l2, amount, lut, canvas, fmt, wt_sink)


def run(gpu, orc, rng, sw, sh, fmt=RGBA, ntracks=1, blend=True, lut=None, order=0, swap=0, wt_src=0, q=2, fix=0, yvu_src=False, pad=(0, 0, 0), tight=False, canvas=None,
        wt_sink=0, yvu_sink=False, pads=(8, 3, 5), srcs=None, dst_off=0, l2_off=0, l2_pad=24):
    """one call with ntracks tracks that all differ; the device buffers are allocated in a shuffled order and handed over in another (slot order != frame order); every
    destination plane is compared whole: frame bytes against the oracle, row padding and guard rows against their fill.  dst_off / l2_off: the address of the (first)
    destination plane / of layer 2 modulo 64.  Chroma planes of the 4:2:0 sink get odd pitches (pads[1], pads[2])."""
    ops = gpu
    cw, ch = (canvas[0], canvas[1]) if canvas else (sw, sh)
    dims = plane_dims(fmt, cw, ch)
    strides = [align(b + pads[k], 4 if fmt != YUV420P else 2 if k == 0 else 1) for k, (b, _) in enumerate(dims)]
    irow2 = align(cw * 4, 4) + l2_pad
    srcs = srcs if srcs is not None else [planes_any(rng, sw, sh, pad, tight) for _ in range(ntracks)]
    l2s = None
    if blend:
        l2s = [rng.integers(0, 256, (ch, irow2), dtype=np.uint8) for _ in range(ntracks)]
        for a in l2s:
            al = a[:, 3:cw * 4:4]
            al[rng.random(al.shape) < 0.5] = 255
    amounts = distinct_amounts(rng, ntracks)
    fills = [[rng.integers(0, 256, (r + GUARD, strides[k]), dtype=np.uint8) for k, (_, r) in enumerate(dims)] for _ in range(ntracks)]
    d_src, d_l2, d_pl = [None] * ntracks, [None] * ntracks, [None] * ntracks
    for i in rng.permutation(ntracks):
        d_pl[i] = [dev_at(f, dst_off if k == 0 else 0) for k, f in enumerate(fills[i])]
        d_src[i] = [dev(p) for p in srcs[i][:3]]
        d_l2[i] = dev_at(l2s[i], l2_off) if blend else None
    slots = [int(k) for k in rng.permutation(ntracks)]
    ssel = [0, 2, 1] if yvu_src else [0, 1, 2]
    dsel = [0, 2, 1] if (yvu_sink and fmt == YUV420P) else list(range(len(dims)))
    ys_, s1, s2 = srcs[0][3]
    stri = (ys_, s2, s1) if yvu_src else (ys_, s1, s2)
    prm = ops.chain_params(sw, sh, 0, sw, sh, irow2, strides[0] if fmt == RGBA else 0, swap_rb=swap, interp=PIXBUF | (0 if blend else NOBLEND), bf=0, lut=lut)
    src = ops.yuv_source(stri, srcs[0][ssel[1]].size, srcs[0][ssel[2]].size, out_order=order, which_tables=wt_src, pb_quality=q, flags=fix)
    am = [amounts[k] for k in slots] if blend else None
    if fmt == RGBA:
        trk = ops.chain_yuv_tracks([d_src[k][0] for k in slots], [d_src[k][ssel[1]] for k in slots], [d_src[k][ssel[2]] for k in slots],
                                   [d_l2[k] for k in slots] if blend else None, [d_pl[k][0] for k in slots])
        ops.chain_flat_yuv420p(prm, src, trk, am, canvas=canvas)
    else:
        assert canvas is None
        sink = ops.chain_sink(fmt, [strides[j] for j in dsel], which_tables=wt_sink, in_order=order ^ swap)
        trk = ops.chain_yuv_sink_tracks([d_src[k][0] for k in slots], [d_src[k][ssel[1]] for k in slots], [d_src[k][ssel[2]] for k in slots],
                                        [d_l2[k] for k in slots] if blend else None, [[d_pl[k][j] for j in dsel] for k in slots])
        ops.chain_flat_yuv420p_to_yuv(prm, src, sink, trk, am)
    wants = []
    for i in range(ntracks):
        want = expected(orc, srcs[i], sw, sh, order, swap, wt_src, q, fix, yvu_src, l2s[i] if blend else None, amounts[i] if blend else 0, lut, canvas, fmt, wt_sink)
        wants.append(want)
        for p, j in enumerate(dsel):              # p: the conversion's plane (Y, U, V); j: the buffer it was handed
            b, r = dims[p]
            got = host(d_pl[i][j])
            bad = got[:r, :b] != want[p][:r, :b]
            assert not bad.any(), "%dx%d fmt %d track %d plane %d: %d bytes differ from the oracle, first at %s" % (sw, sh, fmt, i, p, int(bad.sum()), np.argwhere(bad)[0].tolist())
            assert (got[:r, b:] == fills[i][j][:r, b:]).all(), "track %d plane %d: row padding was written" % (i, p)
            assert (got[r:] == fills[i][j][r:]).all(), "track %d plane %d: guard rows were written" % (i, p)
    return wants


FMTS = [RGBA, UYVY, YUYV, YUV420P]
FMT_IDS = ["rgba", "uyvy", "yuyv", "yuv420p"]


@pytest.mark.gpu
@pytest.mark.parametrize("blend", [True, False], ids=["blend", "noblend"])
@pytest.mark.parametrize("with_lut", [True, False], ids=["lut", "nolut"])
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_chain_flat_stages(gpu, orc, blend, with_lut, fmt):
    """every stage combination to every destination (RGBA also into a canvas), two tracks, both settings of swap_rb; out_order, the tables of both ends, pb_quality,
    LGPU_YUV_FIX_EDGES and the plane orders drawn per run"""
    rng = np.random.default_rng(0xF1A7 + fmt * 4 + blend * 2 + with_lut)
    lut = gamma_lut(orc) if with_lut else None
    for i, (sw, sh) in enumerate([(132, 76), (36, 21) if fmt != YUV420P else (36, 22)]):
        for swap in (0, 1):
            for canvas in ([None, (sw + 7, sh + 5, 3, 2)] if fmt == RGBA else [None]):
                wt_sink = int(rng.integers(0, 4)) if fmt == YUV420P else int(rng.integers(0, 2))
                run(gpu, orc, rng, sw, sh, fmt, ntracks=2, blend=blend, lut=lut, order=int(rng.integers(0, 2)), swap=swap, wt_src=int(rng.integers(0, 4)),
                    q=int(rng.integers(1, 4)), fix=int(rng.integers(0, 2)) * FIX_EDGES, yvu_src=bool(i), pad=(3 * i, 5, 1), tight=bool(i), canvas=canvas, wt_sink=wt_sink,
                    yvu_sink=bool(i), pads=(8 * i, 3 + 2 * i, 7))


SMALL = [(2, 1), (2, 2), (2, 3), (4, 2), (6, 5), (130, 7), (132, 76)]      # row 0 alone; + the trailing row; + a row pair; ...; 130: chroma width 65, 132: 66


@pytest.mark.gpu
@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("sw,sh", SMALL)
def test_chain_flat_smallest_frames_rgba(gpu, orc, sw, sh, fix):
    """the walk's smallest frames into RGBA and the packed sinks: row 0 alone, with and without a row pair, with and without the trailing row; tight chroma planes (the
    read one past the end is clamped) and loose ones with odd pitches"""
    rng = np.random.default_rng(0x5A11 + sw * 131 + sh * 2 + fix)
    lut = gamma_lut(orc)
    for tight in (True, False):
        run(gpu, orc, rng, sw, sh, RGBA, blend=True, lut=lut, fix=fix, q=2 + fix, pad=(1, 1, 3), tight=tight, swap=fix)
        run(gpu, orc, rng, sw, sh, UYVY if tight else YUYV, blend=True, lut=lut, fix=fix, q=1 + fix, pad=(3, 1, 1), tight=tight, order=1)


@pytest.mark.gpu
@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("sw,sh", [g for g in SMALL if not g[1] & 1] + [(2, 4)])
def test_chain_flat_smallest_frames_yuv420p(gpu, orc, sw, sh, fix):
    """the 4:2:0 sink on the even heights of the list and 2x4 (one inner row pair between row 0 and the trailing row): unit p feeds chroma row p - 1, the trailing row
    the last one"""
    rng = np.random.default_rng(0x420 + sw * 131 + sh * 2 + fix)
    for tight in (True, False):
        run(gpu, orc, rng, sw, sh, YUV420P, blend=True, lut=gamma_lut(orc), fix=fix, q=2, pad=(1, 3, 1), tight=tight, wt_sink=int(tight) * 2 + fix, pads=(2, 1, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_chain_flat_wide_and_tall(gpu, orc, fmt):
    """1100 pixels: 550 chroma columns, three workgroups along x with the last one partly empty; a frame of width 4 with more units than a launch's workgroup rows
    (each workgroup then walks a run of units) and one with a few units more than workgroups"""
    rng = np.random.default_rng(0x71DE + fmt)
    run(gpu, orc, rng, 1100, 10 if fmt == YUV420P else 9, fmt, blend=True, lut=gamma_lut(orc), tight=True, pad=(0, 1, 1))
    run(gpu, orc, rng, 4, 2 * UNIT_CAP + 6, fmt, blend=True, fix=1, pad=(1, 1, 1))
    run(gpu, orc, rng, 4, 4 * UNIT_CAP + 2, fmt, ntracks=2, blend=False, lut=gamma_lut(orc), pad=(0, 0, 0), tight=True)


@pytest.mark.gpu
@pytest.mark.parametrize("ox", [0, 3, 6])
@pytest.mark.parametrize("oy", [0, 5])
def test_chain_flat_canvas(gpu, orc, ox, oy):
    """even and odd offs_x, offs_y 0 and above; the bars pass through blend and LUT; the bars written by the same call"""
    rng = np.random.default_rng(0xCA + ox * 8 + oy)
    lut = gamma_lut(orc)
    run(gpu, orc, rng, 130, 7, RGBA, ntracks=2, blend=True, lut=lut, canvas=(130 + ox + 3, 7 + oy + 4, ox, oy), swap=1)
    run(gpu, orc, rng, 36, 22, RGBA, ntracks=2, blend=False, lut=lut, canvas=(36 + ox + 1, 22 + oy, ox, oy))


@pytest.mark.gpu
def test_chain_flat_canvas_centred_and_exact(gpu, orc):
    """where letterbox_layer centres the frame (the oracle's own orc_letterbox places it), a canvas the frame fills exactly, and a canvas large enough for several bar
    workgroups"""
    rng = np.random.default_rng(0xCE)
    lut = gamma_lut(orc)
    run(gpu, orc, rng, 36, 21, RGBA, blend=True, lut=lut, canvas=(47, 30, (47 - 36 + 1) >> 1, (30 - 21 + 1) >> 1))
    run(gpu, orc, rng, 36, 21, RGBA, blend=True, lut=lut, canvas=(36, 21, 0, 0))
    run(gpu, orc, rng, 36, 22, RGBA, ntracks=2, blend=True, canvas=(36, 31, 0, 9))                 # bars above and below only
    run(gpu, orc, rng, 64, 40, RGBA, blend=True, lut=lut, canvas=(700, 300, 321, 130), order=1)    # 207,440 bar pixels: 64 workgroups, each walking its stride


@pytest.mark.gpu
@pytest.mark.parametrize("dst_off,l2_off", [(4, 4), (12, 12), (4, 12), (12, 4), (8, 0)])
def test_chain_flat_addresses(gpu, orc, dst_off, l2_off):
    """destination and layer 2 at 4 and 12 mod 16 with pitches of 4 mod 8: 4-byte stores and loads where the address is not a multiple of 8 (alternating rows)"""
    rng = np.random.default_rng(0xADD + dst_off * 16 + l2_off)
    for canvas in (None, (141, 9, 5, 1)):
        run(gpu, orc, rng, 132, 8, RGBA, ntracks=2, blend=True, lut=gamma_lut(orc), canvas=canvas, dst_off=dst_off, l2_off=l2_off, pads=(4 if canvas is None else 8, 0, 0), l2_pad=20 if canvas is None else 16)
    run(gpu, orc, rng, 132, 8, UYVY, blend=True, dst_off=dst_off, l2_off=l2_off, pads=(4, 0, 0), l2_pad=20)
    run(gpu, orc, rng, 132, 8, YUV420P, blend=True, dst_off=dst_off + 2, l2_off=l2_off, pads=(2, 1, 1), l2_pad=20)


def test_address_case_pitches():
    """the pitches of the case above are 4 mod 8, as it says"""
    assert (align(132 * 4 + 4, 4)) % 8 == 4 and (align(141 * 4 + 8, 4)) % 8 == 4 and (align(132 * 4, 4) + 20) % 8 == 4 and (align(141 * 4, 4) + 16) % 8 == 4 and (132 * 2 + 4) % 8 == 4


@pytest.mark.gpu
@pytest.mark.parametrize("ntracks", [1, 7, 16, 33, 64])
def test_chain_flat_tracks(gpu, orc, ntracks):
    """1 .. 64 tracks in one call with distinct amounts and shuffled buffers, to every destination (YUV420P: 32 tracks per launch, so 33 and 64 go as two); RGBA through
    chain_ref.Tracks"""
    rng = np.random.default_rng(0x7AC + ntracks)
    lut = gamma_lut(orc)
    sw, sh = 68, 10
    srcs = [planes_any(rng, sw, sh, (4, 1, 3), False) for _ in range(ntracks)]
    T = Tracks(rng, srcs, sw + 5, sh + 3)
    ys_, s1, s2 = srcs[0][3]
    prm = gpu.chain_params(sw, sh, 0, sw, sh, T.irow2, T.orow, swap_rb=1, interp=PIXBUF, bf=0, lut=lut)
    src = gpu.yuv_source((ys_, s1, s2), srcs[0][1].size, srcs[0][2].size, out_order=0, which_tables=1, pb_quality=2)
    trk = gpu.chain_yuv_tracks([s[0] for s in T.slots(T.d_src)], [s[1] for s in T.slots(T.d_src)], [s[2] for s in T.slots(T.d_src)], T.slots(T.d_l2), T.slots(T.d_dst))
    gpu.chain_flat_yuv420p(prm, src, trk, T.slots(T.amounts), canvas=(sw + 5, sh + 3, 3, 1))
    for i in range(ntracks):
        Y, U, V, st = srcs[i]
        T.check(i, oracle_flat(orc, Y, U, V, st, sw, sh, 0, 1, 1, 2, 0, T.l2s[i], T.amounts[i], lut, (sw + 5, sh + 3, 3, 1))[0], "rgba")
    run(gpu, orc, rng, sw, sh, YUV420P, ntracks=ntracks, blend=True, lut=lut, order=1, wt_src=2, wt_sink=2, yvu_sink=True, pad=(4, 0, 2))
    run(gpu, orc, rng, sw, sh, UYVY, ntracks=ntracks, blend=True, lut=lut, swap=1)
    run(gpu, orc, rng, sw, sh, YUYV, ntracks=ntracks, blend=True, order=1, wt_sink=1, yvu_src=True)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,wt", [(RGBA, 0), (RGBA, 1), (RGBA, 2), (RGBA, 3), (YUV420P, 0), (YUV420P, 1), (YUV420P, 2), (YUV420P, 3), (UYVY, 0), (UYVY, 1), (YUYV, 0), (YUYV, 1)])
def test_chain_flat_tables(gpu, orc, fmt, wt):
    """all four table sets on the source (through RGBA, every pb_quality) and every valid table set of every sink, behind sources of both byte orders"""
    rng = np.random.default_rng(0x7AB + fmt * 4 + wt)
    if fmt == RGBA:
        for q in (1, 2, 3):
            run(gpu, orc, rng, 132, 21, RGBA, blend=True, lut=gamma_lut(orc), wt_src=wt, q=q, tight=True, pad=(1, 1, 3), fix=q & 1)
    else:
        for order in (0, 1):
            run(gpu, orc, rng, 132, 22, fmt, ntracks=2, blend=True, order=order, wt_src=wt ^ 1, wt_sink=wt, pad=(0, 2, 6))


def test_yuyv_lost_upper_clamp_expectation(orc):
    """the oracle's side of the next test alone: a saturated blue / red frame behind a threshold LUT makes U / V raw 256 with unclamped sink tables, which rgb2yuyv
    (only the lower chroma clamp survives) stores as byte 0 where rgb2uyvy stores 255"""
    lut = np.where(np.arange(256) >= 128, 255, 0).astype(np.uint8)
    for (y, u, v), ch in (((60, 255, 100), 0), ((80, 90, 255), 1)):
        src = flat_planes(24, 6, y, u, v)
        w_yuyv = expected(orc, src, 24, 6, 0, 0, 1, 2, 0, False, None, 0, lut, None, YUYV, 1)[0]
        w_uyvy = expected(orc, src, 24, 6, 0, 0, 1, 2, 0, False, None, 0, lut, None, UYVY, 1)[0]
        assert (w_yuyv[:, 1 + 2 * ch::4] == 0).all() and (w_uyvy[:, 2 * ch::4] == 255).all()
        assert (w_yuyv[:, 0::2] == w_uyvy[:, 1::2]).all()          # luma agrees


@pytest.mark.gpu
def test_chain_flat_yuyv_lost_upper_clamp(gpu, orc):
    """YUYV's missing upper chroma clamp (the expectation is shown to carry the quirk by the test above)"""
    rng = np.random.default_rng(0x10C)
    lut = np.where(np.arange(256) >= 128, 255, 0).astype(np.uint8)
    for y, u, v in ((60, 255, 100), (80, 90, 255)):
        src = flat_planes(24, 6, y, u, v)
        for fmt in (YUYV, UYVY):
            run(gpu, orc, rng, 24, 6, fmt, blend=False, lut=lut, wt_src=1, wt_sink=1, srcs=[src])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [RGBA, UYVY, YUV420P], ids=["rgba", "uyvy", "yuv420p"])
def test_chain_flat_at_size_matches_todays_launches(gpu, orc, fmt):
    """16 x 1920x1080 with blend and gamma: byte-identical to the device's own launches (lgpu_yuv420p_to_rgb_batch, lgpu_chain_amounts, lgpu_rgb_to_yuv_batch) on the same
    inputs; track 0 also against the oracle"""
    import torch
    ops = gpu
    rng = np.random.default_rng(0x51 + fmt)
    w, h, n = 1920, 1080, 16
    lut = gamma_lut(orc)
    g = torch.Generator(device="cuda")
    g.manual_seed(8642 + fmt)
    Ys = [torch.randint(0, 256, (h, w), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    Us = [torch.randint(0, 256, (h // 2, w // 2), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    Vs = [torch.randint(0, 256, (h // 2, w // 2), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    L2 = [torch.randint(0, 256, (h, w * 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    amounts = [int(x) for x in rng.integers(0, 256, n)]
    dims = plane_dims(fmt, w, h)
    fused = [[torch.full((r, b), 0x5C, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
    prm = ops.chain_params(w, h, w * 4, w, h, w * 4, w * 4, swap_rb=1, interp=PIXBUF, bf=0, lut=lut)
    src = ops.yuv_source((w, w // 2, w // 2), Us[0].numel(), Vs[0].numel(), out_order=0, which_tables=0, pb_quality=2)
    if fmt == RGBA:
        ops.chain_flat_yuv420p(prm, src, ops.chain_yuv_tracks(Ys, Us, Vs, L2, [f[0] for f in fused]), amounts)
    else:
        ops.chain_flat_yuv420p_to_yuv(prm, src, ops.chain_sink(fmt, [b for (b, _) in dims], which_tables=0, in_order=1), ops.chain_yuv_sink_tracks(Ys, Us, Vs, L2, fused), amounts)
    conv = [torch.zeros((h, w * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    rgba = [torch.zeros((h, w * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    ops.yuv420p_to_rgb_batch(list(zip(Ys, Us, Vs, conv)), w, h, 4, 0, 0, 0, 2)
    ops.chain_amounts(prm, ops.chain_tracks(conv, L2, rgba), amounts)
    today = [[r] for r in rgba]
    if fmt != RGBA:
        today = [[torch.full((r, b), 0xC5, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
        ops.rgb_to_yuv_batch(rgba, today, w, h, 1, 1, fmt, 0, 0)
    torch.cuda.synchronize()
    for i in range(n):
        for p in range(len(dims)):
            assert torch.equal(fused[i][p], today[i][p]), "track %d plane %d: %d bytes differ from today's launches" % (i, p, int((fused[i][p] != today[i][p]).sum()))
    l2 = host(L2[0])
    want = oracle_flat(orc, host(Ys[0]), host(Us[0]).reshape(-1), host(Vs[0]).reshape(-1), (w, w // 2, w // 2), w, h, 0, 1, 0, 2, 0, l2, amounts[0], lut, None, fmt, 0)
    for p, (b, r) in enumerate(dims):
        assert (host(fused[0][p]) == want[p][:r, :b]).all(), "track 0 plane %d differs from the oracle" % p


@pytest.mark.gpu
def test_chain_flat_refusals(gpu):
    """bad arguments -- every one either 2:1 parent refuses, an odd sw, a destination plane that is a source plane: LGPU_E_BADARG; shapes off the one-launch form:
    LGPU_E_UNSUPPORTED; nothing is written in either case; the same call inside the form runs"""
    import torch
    from lives_amd import lib
    ops = gpu
    w, h = 128, 72
    Y = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    U = torch.zeros((h // 2, w // 2), dtype=torch.uint8, device="cuda")
    V = torch.zeros_like(U)
    L2 = torch.zeros((h + 16, w * 4 + 64), dtype=torch.uint8, device="cuda")
    D = [torch.full((h + 16, w * 4 + 64), 0x5C, dtype=torch.uint8, device="cuda") for _ in range(3)]

    def call(fmt=YUV420P, sw_=w, sh_=h, dw_=None, dh_=None, interp=PIXBUF, blur=0, amounts=(9,), ntracks=1, null_src=False, null_plane=False, strides=(w, w // 2, w // 2),
             usz=None, vsz=None, order=0, swap=0, wt_src=0, q=2, flags=0, wt=0, in_order=None, orow=None, irow2=w * 4 + 64, dst_off=0, l2_off=0, in_place=None, canvas=None):
        dw_, dh_ = sw_ if dw_ is None else dw_, sh_ if dh_ is None else dh_
        orow = orow if orow is not None else [w * 4 + 64] * 3
        prm = ops.chain_params(sw_, sh_, 0, dw_, dh_, irow2, orow[0], swap_rb=swap, interp=interp, do_blur=blur, bf=0)
        src = ops.yuv_source(strides, U.numel() if usz is None else usz, V.numel() if vsz is None else vsz, out_order=order, which_tables=wt_src, pb_quality=q, flags=flags)
        m = max(ntracks, 1)
        if fmt == RGBA:
            trk = ops.chain_yuv_tracks([Y] * m, [U] * m, [V] * m, [L2] * m, [D[0]] * m)
            for t in trk:
                t.dst_d += dst_off
                t.layer2_d += l2_off
            if null_src:
                trk[0].u_d = None
            if null_plane:
                trk[0].dst_d = None
            if in_place is not None:
                trk[0].dst_d = (Y, U, V)[in_place[1]].data_ptr()
            if ntracks < 1:
                trk = (lib.ChainYuvTrack * 0)()
            return ops.chain_flat_yuv420p(prm, src, trk, list(amounts) * m if amounts is not None else None, canvas=canvas, check=False)
        sink = ops.chain_sink(fmt, orow, which_tables=wt, in_order=(order ^ swap) if in_order is None else in_order)
        trk = ops.chain_yuv_sink_tracks([Y] * m, [U] * m, [V] * m, [L2] * m, [D] * m)
        for t in trk:
            t.dst_d[0] += dst_off
            t.layer2_d += l2_off
        if null_src:
            trk[0].u_d = None
        if null_plane:
            trk[0].dst_d[2] = None
        if in_place is not None:
            trk[0].dst_d[in_place[0]] = (Y, U, V)[in_place[1]].data_ptr()
        if ntracks < 1:
            trk = (lib.ChainYuvSinkTrack * 0)()
        return ops.chain_flat_yuv420p_to_yuv(prm, src, sink, trk, list(amounts) * m if amounts is not None else None, check=False)

    source_badarg = {
        "no PIXBUF": dict(interp=3),
        "null amounts with a blend": dict(amounts=None),
        "no tracks": dict(ntracks=0),
        "65 tracks": dict(ntracks=65),
        "null source plane": dict(null_src=True),
        "null destination plane": dict(null_plane=True),
        "out_order 2": dict(order=2, in_order=0),
        "source which_tables 4": dict(wt_src=4),
        "pb_quality 0": dict(q=0),
        "pb_quality 4": dict(q=4),
        "unknown flag": dict(flags=2),
        "luma stride below the width": dict(strides=(w - 4, w // 2, w // 2)),
        "chroma stride below the width": dict(strides=(w, w // 2 - 2, w // 2)),
        "chroma plane too small": dict(usz=U.numel() - 1),
        "odd sw": dict(sw_=127),
        "sw 0": dict(sw_=0),
        "sh 0": dict(sh_=0),
        "dw 0": dict(dw_=0),
        "layer-2 stride below the row": dict(irow2=w * 4 - 8),
        "layer-2 stride not a multiple of 4": dict(irow2=w * 4 + 62),
        "layer 2 not 4-byte aligned": dict(l2_off=2),
        "destination is the source's luma plane": dict(in_place=(0, 0)),
        "destination is a source chroma plane": dict(in_place=(0, 2)),
    }
    rgba_badarg = {
        "destination stride below the row": dict(orow=[w * 4 - 4] * 3),
        "destination stride not a multiple of 4": dict(orow=[w * 4 + 2] * 3),
        "destination not 4-byte aligned": dict(dst_off=2),
        "canvas smaller than the frame": dict(canvas=(w - 2, h, 0, 0)),
        "frame past the canvas": dict(canvas=(w + 4, h + 4, 5, 0)),
        "negative canvas offset": dict(canvas=(w + 4, h + 4, 0, -1)),
        "destination stride below the canvas row": dict(canvas=(w + 32, h, 0, 0)),
    }
    sink_badarg = {
        "out_fmt 1": dict(fmt=1),
        "out_fmt 6": dict(fmt=6),
        "in_order 2": dict(in_order=2),
        "sink which_tables 4": dict(wt=4),
        "BT.709 with UYVY": dict(fmt=UYVY, wt=2),
        "BT.709 with YUYV": dict(fmt=YUYV, wt=3),
        "sink luma stride below the row": dict(orow=[w - 8, w, w]),
        "sink chroma stride below the row": dict(orow=[w, w // 2 - 4, w]),
        "packed stride below the row": dict(fmt=UYVY, orow=[w * 2 - 8, 0, 0]),
        "in_order against the chain's (no swap)": dict(order=1, swap=0, in_order=0),
        "in_order against the chain's (swap)": dict(order=1, swap=1, in_order=1),
        "chroma sink plane is a source chroma plane": dict(in_place=(1, 2)),
    }
    common_unsupported = {
        "2:1": dict(dw_=w // 2, dh_=h // 2),
        "another width": dict(dw_=w + 2),
        "another height": dict(dh_=h - 1),
        "gaussian": dict(blur=1),
        "luma plane of 2 GiB": dict(strides=(1 << 25, w // 2, w // 2)),
        "chroma plane of 2 GiB": dict(usz=1 << 31),
    }
    sink_unsupported = {
        "YUV422P": dict(fmt=5),
        "odd dh with 4:2:0": dict(sh_=71),
        "odd luma rowstride": dict(orow=[w + 1, w, w]),
        "odd luma plane": dict(dst_off=1),
        "packed rowstride % 4 == 2": dict(fmt=YUYV, orow=[w * 2 + 2, 0, 0]),
        "packed plane at 2 mod 4": dict(fmt=UYVY, dst_off=2),
    }
    cases = []
    for fmt in (RGBA, YUV420P):
        for what, kw in source_badarg.items():
            cases.append((what, dict(fmt=fmt, **kw), E_BADARG))
        for what, kw in common_unsupported.items():
            cases.append((what, dict(fmt=fmt, **kw), E_UNSUPPORTED))
    cases += [(what, dict(fmt=RGBA, **kw), E_BADARG) for what, kw in rgba_badarg.items()]
    cases += [(what, kw, E_BADARG) for what, kw in sink_badarg.items()]
    cases += [(what, kw, E_UNSUPPORTED) for what, kw in sink_unsupported.items()]
    for what, kw, want in cases:
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc == want, "%s (%s): %d, expected %d (%s)" % (what, kw, rc, want, lib.load().lgpu_last_error())
        assert all(bool((d == 0x5C).all()) for d in D), "%s: a destination plane was written" % what
        if what == "2:1":
            name = b"lgpu_chain_yuv420p_to_yuv" if kw["fmt"] != RGBA else b"lgpu_chain_yuv420p"
            assert name in lib.load().lgpu_last_error().split(b": ", 1)[1], "the refusal does not name the 2:1 entry point"
    # ... and the same calls inside the form run
    assert call(fmt=UYVY, sh_=71) == 0                 # any height for the packed formats
    torch.cuda.synchronize()
    assert not bool((D[0][:71, :w * 2] == 0x5C).all()) and bool((D[0][71:] == 0x5C).all()) and bool((D[1] == 0x5C).all())
    assert call(order=1, swap=1) == 0
    torch.cuda.synchronize()
    assert not bool((D[0][:h, :w] == 0x5C).all()) and not any(bool((d[:h // 2, :w // 2] == 0x5C).all()) for d in D[1:])
    for d in D:
        d.fill_(0x5C)
    assert call(fmt=RGBA, sh_=71, canvas=(w + 8, h, 3, 1)) == 0
    torch.cuda.synchronize()
    assert not bool((D[0][:h, :(w + 8) * 4] == 0x5C).all()) and bool((D[0][h:] == 0x5C).all()) and bool((D[0][:, (w + 8) * 4:] == 0x5C).all())
