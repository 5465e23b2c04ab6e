"""lgpu_chain_flat_yuv422: the UNSCALED tick from 4:2:2 frames -- planar YUV422P, packed UYVY / YUYV -- as one launch (K2's 4:2:2 walk or K3's macropixel conversion ->
[R <-> B] -> [letterbox] -> [chroma blend] -> [gamma LUT] -> RGBA, or -> K4's conversion to UYVY / YUYV / YUV420P; no RGBA frame in between) against the oracle's
composition orc_yuv420p_to_rgb(is_422 = 1) or orc_yuv_to_rgb(in_fmt 2 / 3) -> the stages of tests/test_chain_flat.py's oracle_flat; at size against the device's own
launches; and the refusals.  Bit-exact: every byte of every destination plane, and every byte of the planes' row padding and guard rows."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.chain_ref import BLACK, distinct_amounts
from tests.offset_buffers import dev_at
from tests.test_chain_flat import GUARD, UNIT_CAP, gamma_lut, plane_dims
from tests.util import align, dev, host

P = po.P
PIXBUF, NOBLEND = 0x100, 0x400
E_BADARG, E_UNSUPPORTED = -2, -3
RGBA, UYVY, YUYV, YUV420P, YUV422P = 0, 2, 3, 4, 5
SRCS = [YUV422P, UYVY, YUYV]
SRC_IDS = ["yuv422p", "uyvy", "yuyv"]


def source(rng, sfmt, sw, sh, pad=(0, 0, 0), tight=False):
    """one 4:2:2 frame as a list of host planes (2-D luma / packed rows, 1-D chroma).  YUV422P: chroma rows of sw / 2 + pad[1] / pad[2] bytes, sh of them; tight: each
    chroma plane ends with its last sample, so that the walk's read one past the last row's end is clamped to the plane's last byte.  Packed: rows of 2 sw + pad[0]
    bytes (pad[0] a multiple of 4)"""
    if sfmt != YUV422P:
        assert pad[0] % 4 == 0
        return [rng.integers(0, 256, (sh, sw * 2 + pad[0]), dtype=np.uint8)]
    hw = sw // 2
    us, vs = hw + pad[1], hw + pad[2]
    return [rng.integers(0, 256, (sh, sw + pad[0]), dtype=np.uint8),
            rng.integers(0, 256, (sh - 1) * us + hw if tight else sh * us, dtype=np.uint8),
            rng.integers(0, 256, (sh - 1) * vs + hw if tight else sh * vs, dtype=np.uint8)]


def strides_of(sfmt, sw, pl, pad):
    return (pl[0].strides[0], sw // 2 + pad[1], sw // 2 + pad[2]) if sfmt == YUV422P else (pl[0].strides[0],)


def first_stage(orc, sfmt, pl, strides, sw, sh, order, wt, q, is_422=1):
    """the tight RGBA frame the chain starts from: lgpu_yuv420p_to_rgb(is_422) / lgpu_yuv_to_rgb as the oracle has them"""
    rgba = np.zeros((sh, sw * 4), np.uint8)
    if sfmt == YUV422P:
        st = (ctypes.c_int * 3)(*strides)
        orc.orc_yuv420p_to_rgb(P(pl[0]), P(pl[1]), P(pl[2]), st, pl[1].size, pl[2].size, P(rgba), sw * 4, sw, sh, 4, order, is_422, wt, q, None, 0)
    else:
        sp, ss = po.planes_args(pl)
        assert orc.orc_yuv_to_rgb(ctypes.addressof(sp), ctypes.addressof(ss), sw, sh, sfmt, 0, P(rgba), sw * 4, order, 1, wt) == 0
    return rgba


def oracle_tail(orc, rgba, sw, sh, order, swap, l2, amount, lut, canvas=None, fmt=RGBA, wt_sink=0):
    """the stages of test_chain_flat.oracle_flat behind its conversion, on a tight RGBA frame: the list of destination planes one track must equal"""
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


def run(gpu, orc, rng, sfmt, sw, sh, fmt=RGBA, ntracks=1, blend=True, lut=None, order=0, swap=0, wt_src=0, q=2, pad=(0, 0, 0), tight=False, canvas=None, wt_sink=0,
        pads=(8, 3, 5), dst_off=0, l2_off=0, l2_pad=24, src_off=(0, 0, 0)):
    """one call with ntracks tracks that all differ, buffers allocated in a shuffled order and handed over in another; every destination plane is compared whole: frame
    bytes against the oracle, row padding and guard rows against their fill (tests/test_chain_flat.py's run, from a 4:2:2 source).  src_off: the address of each source
    plane modulo 64"""
    ops = gpu
    cw, ch = (canvas[0], canvas[1]) if canvas else (sw, sh)
    dims = plane_dims(fmt, cw, ch)
    strides = [align(b + pads[k], 4 if fmt != YUV420P else 2 if k == 0 else 1) for k, (b, _) in enumerate(dims)]
    irow2 = align(cw * 4, 4) + l2_pad
    srcs = [source(rng, sfmt, sw, sh, pad, tight) for _ in range(ntracks)]
    stri = strides_of(sfmt, sw, srcs[0], pad)
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
        d_src[i] = [dev_at(p if p.ndim == 2 else p.reshape(1, -1), src_off[k]) for k, p in enumerate(srcs[i])]
        d_l2[i] = dev_at(l2s[i], l2_off) if blend else None
    slots = [int(k) for k in rng.permutation(ntracks)]
    prm = ops.chain_params(sw, sh, 0, sw, sh, irow2, strides[0] if fmt == RGBA else 0, swap_rb=swap, interp=PIXBUF | (0 if blend else NOBLEND), bf=0, lut=lut)
    planar_src = sfmt == YUV422P
    src = ops.yuv422_source(sfmt, stri, srcs[0][1].size if planar_src else 0, srcs[0][2].size if planar_src else 0, out_order=order, which_tables=wt_src, pb_quality=q)
    sink = ops.chain_sink(fmt, strides, which_tables=wt_sink, in_order=order ^ swap) if fmt != RGBA else None
    trk = ops.chain_yuv_sink_tracks([d_src[k][0] for k in slots], [d_src[k][1] for k in slots] if planar_src else None, [d_src[k][2] for k in slots] if planar_src else None,
                                    [d_l2[k] for k in slots] if blend else None, [d_pl[k] for k in slots])
    ops.chain_flat_yuv422(prm, src, trk, [amounts[k] for k in slots] if blend else None, sink=sink, canvas=canvas)
    for i in range(ntracks):
        rgba = first_stage(orc, sfmt, srcs[i], stri, sw, sh, order, wt_src, q)
        want = oracle_tail(orc, rgba, sw, sh, order, swap, l2s[i] if blend else None, amounts[i] if blend else 0, lut, canvas, fmt, wt_sink)
        for p, (b, r) in enumerate(dims):
            got = host(d_pl[i][p])
            bad = got[:r, :b] != want[p][:r, :b]
            assert not bad.any(), "src %d %dx%d fmt %d track %d plane %d: %d bytes differ from the oracle, first at %s" % (
                sfmt, sw, sh, fmt, i, p, int(bad.sum()), np.argwhere(bad)[0].tolist())
            assert (got[:r, b:] == fills[i][p][:r, b:]).all(), "track %d plane %d: row padding was written" % (i, p)
            assert (got[r:] == fills[i][p][r:]).all(), "track %d plane %d: guard rows were written" % (i, p)


FMTS = [RGBA, UYVY, YUYV, YUV420P]
FMT_IDS = ["rgba", "uyvy", "yuyv", "yuv420p"]


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_yuv422_source_struct_and_symbol():
    """lgpu_yuv422_source as include/lives_gpu.h lays it out (int, int[3], long, long, int, int, int: 48 bytes on LP64) and the entry point in the built library"""
    from lives_amd import lib
    assert ctypes.sizeof(lib.Yuv422Source) == 48 and lib.Yuv422Source.u_size.offset == 16 and lib.Yuv422Source.out_order.offset == 32
    assert "lgpu_chain_flat_yuv422" in lib.PROTOTYPES and len(lib.PROTOTYPES["lgpu_chain_flat_yuv422"]) == 8
    assert hasattr(lib.load(), "lgpu_chain_flat_yuv422")


def test_oracle_tail_is_oracle_flats_tail(orc):
    """oracle_tail above restates the stages tests/test_chain_flat.py's oracle_flat runs behind its conversion (they cannot be imported apart from it): on a 4:2:0 frame,
    where both exist, the conversion followed by oracle_tail gives oracle_flat's planes -- with swap, canvas (centred and not), blend, table, and to every sink"""
    from tests.test_chain_flat import oracle_flat, planes_any
    rng = np.random.default_rng(0x7A11)
    sw, sh = 36, 22
    Y, U, V, st = planes_any(rng, sw, sh, (3, 1, 5), False)
    lut = gamma_lut(orc)
    for fmt, canvas, swap, order in ((RGBA, None, 0, 0), (RGBA, (sw + 7, sh + 5, 3, 1), 1, 1), (RGBA, (47, 30, (47 - sw + 1) >> 1, (30 - sh + 1) >> 1), 0, 1), (UYVY, None, 1, 0),
                                     (YUYV, None, 0, 1), (YUV420P, None, 1, 1)):
        cw, ch = (canvas[0], canvas[1]) if canvas else (sw, sh)
        l2 = rng.integers(0, 256, (ch, cw * 4 + 8), dtype=np.uint8)
        rgba = np.zeros((sh, sw * 4), np.uint8)
        orc.orc_yuv420p_to_rgb(P(Y), P(U), P(V), (ctypes.c_int * 3)(*st), U.size, V.size, P(rgba), sw * 4, sw, sh, 4, order, 0, 1, 2, None, 0)
        mine = oracle_tail(orc, rgba, sw, sh, order, swap, l2, 77, lut, canvas, fmt, 1)
        theirs = oracle_flat(orc, Y, U, V, st, sw, sh, order, swap, 1, 2, 0, l2, 77, lut, canvas, fmt, 1)
        assert len(mine) == len(theirs) and all((a == b).all() for a, b in zip(mine, theirs)), (fmt, canvas)


def test_422_expectation_is_not_the_420_one_and_carries_the_seed(orc):
    """the frames the GPU tests draw tell the walks apart: the oracle's 4:2:2 answer differs from its 4:2:0 answer on the same planes, and columns 0 / 1 of a row
    i >= 2 depend on chroma row i >> 1 (the reference's seed), not only on row i"""
    rng = np.random.default_rng(0x422)
    sw, sh = 8, 5
    pl = source(rng, YUV422P, sw, sh, (1, 1, 3))
    st = strides_of(YUV422P, sw, pl, (1, 1, 3))
    right = first_stage(orc, YUV422P, pl, st, sw, sh, 0, 0, 2)
    as420 = first_stage(orc, YUV422P, pl, st, sw, sh, 0, 0, 2, is_422=0)
    assert (right != as420).any(), "the 4:2:2 and 4:2:0 readings of these planes agree: a kernel on the wrong walk would pass"
    i = 4                                   # seeded from chroma row 2
    other = [pl[0], pl[1].copy(), pl[2].copy()]
    for p, s in ((1, st[1]), (2, st[2])):
        other[p][(i >> 1) * s] ^= 0x80      # U[2][0], V[2][0]
    moved = first_stage(orc, YUV422P, other, st, sw, sh, 0, 0, 2)
    assert (moved[i, :16] != right[i, :16]).any(), "row %d's first pixels do not depend on chroma row %d: the expectation carries no seed" % (i, i >> 1)
    assert (moved[i, 16:] == right[i, 16:]).all() and (moved[3] == right[3]).all(), "the seed reaches further than cells 0 and 1"
    # packed: the two formats read the same bytes differently
    fr = source(rng, UYVY, sw, sh, (4, 0, 0))
    assert (first_stage(orc, UYVY, fr, None, sw, sh, 0, 0, 2) != first_stage(orc, YUYV, fr, None, sw, sh, 0, 0, 2)).any()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("blend", [True, False], ids=["blend", "noblend"])
@pytest.mark.parametrize("with_lut", [True, False], ids=["lut", "nolut"])
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("sfmt", SRCS, ids=SRC_IDS)
def test_chain_flat422_stages(gpu, orc, sfmt, blend, with_lut, fmt):
    """every stage combination from every source to every destination (RGBA also into a canvas at an odd offset), two tracks, both settings of swap_rb; out_order, the
    tables of both ends and pb_quality drawn per run"""
    rng = np.random.default_rng(0x4227 + sfmt * 64 + fmt * 4 + blend * 2 + with_lut)
    lut = gamma_lut(orc) if with_lut else None
    for i, (sw, sh) in enumerate([(132, 76), (36, 21) if fmt != YUV420P else (36, 22)]):
        for swap in (0, 1):
            for canvas in ([None, (sw + 7, sh + 5, 3, 1)] if fmt == RGBA else [None]):
                wt_sink = int(rng.integers(0, 4)) if fmt == YUV420P else int(rng.integers(0, 2))
                run(gpu, orc, rng, sfmt, sw, sh, fmt, ntracks=2, blend=blend, lut=lut, order=int(rng.integers(0, 2)), swap=swap,
                    wt_src=int(rng.integers(0, 4 if sfmt == YUV422P else 2)), q=int(rng.integers(1, 4)), pad=(4 * i, 5, 1), tight=bool(i), canvas=canvas, wt_sink=wt_sink,
                    pads=(8 * i, 3 + 2 * i, 7))


# widths 2, 4, 6, 8: k = 0 seeded from row i >> 1; k = 1 with a seeded lu; the first regular k; the first 4-byte window.  Heights 1 .. 5: rows with i >> 1 != i exist from 2 on
SMALL = [(w, h) for w in (2, 4, 6, 8) for h in (1, 2, 3, 4, 5)] + [(130, 7), (132, 76)]


@pytest.mark.gpu
@pytest.mark.parametrize("sfmt", SRCS, ids=SRC_IDS)
@pytest.mark.parametrize("sw,sh", SMALL)
def test_chain_flat422_smallest_frames(gpu, orc, sfmt, sw, sh):
    """the walk's smallest frames to RGBA and the packed sinks, and on the even heights to YUV420P; tight chroma planes (the last row's k + 1 read is clamped to the
    plane's last byte) and loose ones with odd pitches; packed rows with padding"""
    rng = np.random.default_rng(0x5A22 + sfmt * 4096 + sw * 131 + sh)
    lut = gamma_lut(orc)
    for tight in (True, False):
        pad = (0 if tight else 4, 1, 3)
        run(gpu, orc, rng, sfmt, sw, sh, RGBA, blend=True, lut=lut, pad=pad, tight=tight, swap=int(tight), q=1 + int(tight))
        run(gpu, orc, rng, sfmt, sw, sh, UYVY if tight else YUYV, blend=True, lut=lut, pad=pad, tight=tight, order=1, wt_src=1)
        if not sh & 1:
            run(gpu, orc, rng, sfmt, sw, sh, YUV420P, blend=True, lut=lut, pad=pad, tight=tight, wt_sink=int(tight) * 2 + 1, pads=(2, 1, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("sfmt", [YUV422P, UYVY], ids=["yuv422p", "uyvy"])
def test_chain_flat422_wide_and_tall(gpu, orc, sfmt, fmt):
    """1100 pixels: 550 cells per row, three workgroups along x with the last one partly empty; frames of width 4 with more units than a launch's workgroup rows (each
    workgroup then walks a run of units)"""
    rng = np.random.default_rng(0x71D2 + sfmt * 8 + fmt)
    run(gpu, orc, rng, sfmt, 1100, 10 if fmt == YUV420P else 9, fmt, blend=True, lut=gamma_lut(orc), tight=True, pad=(0, 1, 1))
    run(gpu, orc, rng, sfmt, 4, 2 * UNIT_CAP + 6, fmt, blend=True, pad=(4, 1, 1))
    run(gpu, orc, rng, sfmt, 4, 4 * UNIT_CAP + 2, fmt, ntracks=2, blend=False, lut=gamma_lut(orc), tight=True)


@pytest.mark.gpu
@pytest.mark.parametrize("ntracks", [1, 7, 16, 32, 33, 64])
@pytest.mark.parametrize("sfmt", [YUV422P, YUYV], ids=["yuv422p", "yuyv"])
def test_chain_flat422_tracks(gpu, orc, sfmt, ntracks):
    """1 .. 64 tracks in one call with distinct amounts and shuffled slots, to RGBA (into a canvas) and to YUV420P (32 tracks per launch: 33 and 64 go as two)"""
    rng = np.random.default_rng(0x7A22 + sfmt * 128 + ntracks)
    lut = gamma_lut(orc)
    sw, sh = 68, 10
    run(gpu, orc, rng, sfmt, sw, sh, RGBA, ntracks=ntracks, blend=True, lut=lut, swap=1, wt_src=1, pad=(4, 1, 3), canvas=(sw + 5, sh + 3, 3, 1))
    run(gpu, orc, rng, sfmt, sw, sh, YUV420P, ntracks=ntracks, blend=True, lut=lut, order=1, wt_sink=2, pad=(4, 0, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("dst_off,l2_off", [(4, 4), (12, 4), (4, 0), (12, 0)])
def test_chain_flat422_addresses(gpu, orc, dst_off, l2_off):
    """destination at 4 and 12 mod 16 and layer 2 at 4, with pitches of 4 mod 8 (4-byte stores and loads on alternating rows); a packed source at every multiple of 4
    modulo 16; the planar source's planes at odd addresses"""
    rng = np.random.default_rng(0xAD22 + dst_off * 16 + l2_off)
    for sfmt, src_off in ((YUV422P, (1, 3, 7)), (YUV422P, (0, 5, 2)), (UYVY, (0, 0, 0)), (UYVY, (4, 0, 0)), (YUYV, (8, 0, 0)), (YUYV, (12, 0, 0))):
        run(gpu, orc, rng, sfmt, 132, 8, RGBA, ntracks=2, blend=True, lut=gamma_lut(orc), dst_off=dst_off, l2_off=l2_off, pads=(4, 0, 0), l2_pad=20, src_off=src_off, pad=(4, 1, 0))
        run(gpu, orc, rng, sfmt, 132, 8, UYVY, blend=True, dst_off=dst_off, l2_off=l2_off, pads=(4, 0, 0), l2_pad=20, src_off=src_off, pad=(0, 0, 3))
        run(gpu, orc, rng, sfmt, 132, 8, YUV420P, blend=True, dst_off=dst_off + 2, l2_off=l2_off, pads=(2, 1, 1), l2_pad=20, src_off=src_off)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [RGBA, UYVY, YUV420P], ids=["rgba", "uyvy", "yuv420p"])
@pytest.mark.parametrize("sfmt", [YUV422P, UYVY], ids=["yuv422p", "uyvy"])
def test_chain_flat422_at_size_matches_todays_launches(gpu, orc, sfmt, fmt):
    """2 x 1920x1080 with blend and gamma: byte-identical to the device's own launches (lgpu_yuv420p_to_rgb_batch with is_422 or lgpu_yuv_to_rgb_batch, lgpu_chain_amounts,
    lgpu_rgb_to_yuv_batch) on the same inputs"""
    import torch
    ops = gpu
    rng = np.random.default_rng(0x51 + sfmt * 8 + fmt)
    w, h, n = 1920, 1080, 2
    lut = gamma_lut(orc)
    g = torch.Generator(device="cuda")
    g.manual_seed(4220 + sfmt * 8 + fmt)
    rnd = lambda r, b: torch.randint(0, 256, (r, b), dtype=torch.uint8, device="cuda", generator=g)
    L2 = [rnd(h, w * 4) for _ in range(n)]
    amounts = [int(x) for x in rng.integers(1, 255, n)]
    dims = plane_dims(fmt, w, h)
    fused = [[torch.full((r, b), 0x5C, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
    conv = [torch.zeros((h, w * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    prm = ops.chain_params(w, h, w * 4, w, h, w * 4, w * 4, swap_rb=1, interp=PIXBUF, bf=0, lut=lut)
    sink = ops.chain_sink(fmt, [b for (b, _) in dims], which_tables=0, in_order=1) if fmt != RGBA else None
    if sfmt == YUV422P:
        Ys, Us, Vs = [rnd(h, w) for _ in range(n)], [rnd(h, w // 2) for _ in range(n)], [rnd(h, w // 2) for _ in range(n)]
        src = ops.yuv422_source(YUV422P, (w, w // 2, w // 2), Us[0].numel(), Vs[0].numel(), out_order=0, which_tables=0, pb_quality=2)
        ops.chain_flat_yuv422(prm, src, ops.chain_yuv_sink_tracks(Ys, Us, Vs, L2, fused), amounts, sink=sink)
        ops.yuv420p_to_rgb_batch(list(zip(Ys, Us, Vs, conv)), w, h, 4, 0, 1, 0, 2)
    else:
        Fs = [rnd(h, w * 2) for _ in range(n)]
        src = ops.yuv422_source(sfmt, (w * 2,), out_order=0, which_tables=0)
        ops.chain_flat_yuv422(prm, src, ops.chain_yuv_sink_tracks(Fs, None, None, L2, fused), amounts, sink=sink)
        ops.yuv_to_rgb_batch([[f] for f in Fs], conv, w, h, sfmt, 0, 0, 1, 0)
    rgba = [torch.zeros((h, w * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    ops.chain_amounts(prm, ops.chain_tracks(conv, L2, rgba), amounts)
    today = [[r] for r in rgba]
    if fmt != RGBA:
        today = [[torch.full((r, b), 0xC5, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
        ops.rgb_to_yuv_batch(rgba, today, w, h, 1, 1, fmt, 0, 0)
    torch.cuda.synchronize()
    for i in range(n):
        for p in range(len(dims)):
            assert torch.equal(fused[i][p], today[i][p]), "track %d plane %d: %d bytes differ from today's launches" % (i, p, int((fused[i][p] != today[i][p]).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("sfmt", SRCS, ids=SRC_IDS)
def test_chain_flat422_refusals(gpu, sfmt):
    """bad arguments: LGPU_E_BADARG; shapes off the one-launch form: LGPU_E_UNSUPPORTED; nothing is written in either case; the same call inside the form runs"""
    import torch
    from lives_amd import lib
    ops = gpu
    w, h = 128, 72
    planar_src = sfmt == YUV422P
    Y = torch.zeros((h, w if planar_src else w * 2), dtype=torch.uint8, device="cuda")
    U = torch.zeros((h, w // 2), dtype=torch.uint8, device="cuda")
    V = torch.zeros_like(U)
    L2 = torch.zeros((h + 16, w * 4 + 64), dtype=torch.uint8, device="cuda")
    D = [torch.full((h + 16, w * 4 + 64), 0x5C, dtype=torch.uint8, device="cuda") for _ in range(3)]
    full = (w, w // 2, w // 2) if planar_src else (w * 2, 0, 0)

    def call(fmt=YUV420P, sw_=w, sh_=h, dw_=None, dh_=None, interp=PIXBUF, blur=0, amounts=(9,), ntracks=1, null_src=None, null_plane=False, strides=full, usz=None, vsz=None,
             order=0, swap=0, wt_src=0, q=2, wt=0, in_order=None, orow=None, irow2=w * 4 + 64, dst_off=0, l2_off=0, src_off=0, in_place=None, canvas=None, in_fmt=sfmt):
        dw_, dh_ = sw_ if dw_ is None else dw_, sh_ if dh_ is None else dh_
        orow = orow if orow is not None else [w * 4 + 64] * 3
        prm = ops.chain_params(sw_, sh_, 0, dw_, dh_, irow2, orow[0], swap_rb=swap, interp=interp, do_blur=blur, bf=0)
        src = ops.yuv422_source(in_fmt, strides, U.numel() if usz is None else usz, V.numel() if vsz is None else vsz, out_order=order, which_tables=wt_src, pb_quality=q)
        m = max(ntracks, 1)
        sink = ops.chain_sink(fmt, orow, which_tables=wt, in_order=(order ^ swap) if in_order is None else in_order) if fmt != RGBA else None
        trk = ops.chain_yuv_sink_tracks([Y] * m, [U] * m if planar_src else None, [V] * m if planar_src else None, [L2] * m, [D] * m)
        for t in trk:
            t.dst_d[0] += dst_off
            t.layer2_d += l2_off
            t.y_d += src_off
        if null_src is not None:
            setattr(trk[0], null_src, None)
        if null_plane:
            trk[0].dst_d[0 if fmt != YUV420P else 2] = None
        if in_place is not None:
            trk[0].dst_d[in_place[0]] = (Y, U, V)[in_place[1]].data_ptr()
        if ntracks < 1:
            trk = (lib.ChainYuvSinkTrack * 0)()
        return ops.chain_flat_yuv422(prm, src, trk, list(amounts) * m if amounts is not None else None, sink=sink, canvas=canvas, check=False)

    badarg = {
        "no PIXBUF": dict(interp=3),
        "null amounts with a blend": dict(amounts=None),
        "no tracks": dict(ntracks=0),
        "65 tracks": dict(ntracks=65),
        "null frame / luma plane": dict(null_src="y_d"),
        "null destination plane": dict(null_plane=True),
        "out_order 2": dict(order=2, in_order=0),
        "source which_tables 4": dict(wt_src=4),
        "pb_quality 0": dict(q=0),
        "pb_quality 4": dict(q=4),
        "in_fmt 4 (YUV420P)": dict(in_fmt=4),
        "in_fmt 0": dict(in_fmt=0),
        "in_fmt 6": dict(in_fmt=6),
        "first stride below the row": dict(strides=(full[0] - 4, full[1], full[2])),
        "odd sw": dict(sw_=127),
        "sw 0": dict(sw_=0),
        "sh 0": dict(sh_=0),
        "dw 0": dict(dw_=0),
        "layer-2 stride below the row": dict(irow2=w * 4 - 8),
        "layer-2 stride not a multiple of 4": dict(irow2=w * 4 + 62),
        "layer 2 not 4-byte aligned": dict(l2_off=2),
        "destination is the frame / luma plane": dict(in_place=(0, 0)),
    }
    if planar_src:
        badarg.update({
            "null U plane": dict(null_src="u_d"),
            "null V plane": dict(null_src="v_d"),
            "chroma stride below the width": dict(strides=(w, w // 2 - 2, w // 2)),
            "chroma plane one byte short": dict(usz=(h - 1) * (w // 2) + w // 2 - 1),
            "chroma plane of 4:2:0 size": dict(vsz=(h // 2) * (w // 2)),
            "destination is a source chroma plane": dict(in_place=(0, 2)),
        })
    else:
        badarg.update({"BT.709 tables with a packed source": dict(wt_src=2), "BT.709 unclamped with a packed source": dict(wt_src=3)})
    rgba_badarg = {
        "destination stride below the row": dict(orow=[w * 4 - 4] * 3),
        "destination stride not a multiple of 4": dict(orow=[w * 4 + 2] * 3),
        "destination not 4-byte aligned": dict(dst_off=2),
        "canvas smaller than the frame": dict(canvas=(w - 2, h, 0, 0)),
        "frame past the canvas": dict(canvas=(w + 4, h + 4, 5, 0)),
        "negative canvas offset": dict(canvas=(w + 4, h + 4, 0, -1)),
    }
    sink_badarg = {
        "a canvas with a sink": dict(canvas=(w, h, 0, 0)),
        "out_fmt 1": dict(fmt=1),
        "out_fmt 6": dict(fmt=6),
        "in_order 2": dict(in_order=2),
        "sink which_tables 4": dict(wt=4),
        "BT.709 with UYVY": dict(fmt=UYVY, wt=2),
        "sink luma stride below the row": dict(orow=[w - 8, w, w]),
        "sink chroma stride below the row": dict(orow=[w, w // 2 - 4, w]),
        "packed stride below the row": dict(fmt=UYVY, orow=[w * 2 - 8, 0, 0]),
        "in_order against the chain's (no swap)": dict(order=1, swap=0, in_order=0),
        "in_order against the chain's (swap)": dict(order=1, swap=1, in_order=1),
    }
    if planar_src:
        sink_badarg["chroma sink plane is a source chroma plane"] = dict(in_place=(1, 2))
    common_unsupported = {
        "2:1": dict(dw_=w // 2, dh_=h // 2),
        "another width": dict(dw_=w + 2),
        "another height": dict(dh_=h - 1),
        "gaussian": dict(blur=1),
        "first plane of 2 GiB": dict(strides=(1 << 25, full[1], full[2])),
    }
    if planar_src:
        common_unsupported["chroma plane of 2 GiB"] = dict(usz=1 << 31)
    else:
        common_unsupported.update({"packed source rowstride % 4 == 2": dict(strides=(w * 2 + 2, 0, 0)), "packed source at 2 mod 4": dict(src_off=2)})
    sink_unsupported = {
        "YUV422P sink": dict(fmt=5),
        "odd dh with 4:2:0": dict(sh_=71),
        "odd luma rowstride": dict(orow=[w + 1, w, w]),
        "odd luma plane": dict(dst_off=1),
        "packed rowstride % 4 == 2": dict(fmt=YUYV, orow=[w * 2 + 2, 0, 0]),
        "packed plane at 2 mod 4": dict(fmt=UYVY, dst_off=2),
    }
    cases = []
    for fmt in (RGBA, YUV420P):
        cases += [(what, dict(fmt=fmt, **kw), E_BADARG) for what, kw in badarg.items()]
        cases += [(what, dict(fmt=fmt, **kw), E_UNSUPPORTED) for what, kw in common_unsupported.items()]
    cases += [(what, dict(fmt=RGBA, **kw), E_BADARG) for what, kw in rgba_badarg.items()]
    cases += [(what, kw, E_BADARG) for what, kw in sink_badarg.items()]
    cases += [(what, kw, E_UNSUPPORTED) for what, kw in sink_unsupported.items()]
    for what, kw, want in cases:
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc == want, "%s (%s): %d, expected %d (%s)" % (what, kw, rc, want, lib.load().lgpu_last_error())
        assert all(bool((d == 0x5C).all()) for d in D), "%s: a destination plane was written" % what
    # ... and the same calls inside the form run
    assert call(fmt=UYVY, sh_=71) == 0                 # any height for the packed sinks
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
