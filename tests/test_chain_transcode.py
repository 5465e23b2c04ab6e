"""lgpu_chain_yuv420p_to_yuv: the 2:1 chain from decoded planar 4:2:0 frames to a YUV sink (K2's conversion in registers -> the exact 2:1 scaler -> [chroma blend] ->
[gamma LUT] -> K4's conversion to UYVY / YUYV / YUV420P in the store, one launch, no RGBA frame at either end) against the oracle's composition
orc_yuv420p_to_rgb -> orc_pixbuf_scale -> [orc_blend_chroma] -> [orc_gamma_apply] -> orc_rgb_to_yuv; at size against the device's own two launches lgpu_chain_yuv420p +
lgpu_rgb_to_yuv_batch; and its refusals.  Bit-exact: every byte of every sink plane, and every byte of the planes' row padding and guard rows."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.chain_ref import distinct_amounts, oracle_chain, planes
from tests.util import align, dev, host

P = po.P
PIXBUF, NOBLEND = 0x100, 0x400
E_BADARG, E_UNSUPPORTED = -2, -3
UYVY, YUYV, YUV420P = 2, 3, 4
FIX_EDGES = 1
GUARD = 2


def gamma_lut(orc):
    lut = np.zeros(256, np.uint8)
    assert orc.orc_gamma_lut8(1.0, po.GAMMA_SRGB, po.GAMMA_LINEAR, 1.4, P(lut)) == 1
    return lut


def plane_dims(fmt, dw, dh):
    """(bytes per row, rows) of the sink's planes"""
    return [(dw * 2, dh)] if fmt in (UYVY, YUYV) else [(dw, dh), (dw >> 1, dh >> 1), (dw >> 1, dh >> 1)]


def oracle_sink(orc, rgba, dw, dh, fmt, in_order, wt):
    """K4 on the chain's RGBA result, into compact planes (the reference's 4:2:0 and UYVY row arithmetic exists on compact rows only)"""
    want, _ = po.k4_out_planes(0, dw, dh, fmt, 0)
    wp, ws = po.planes_args(want)
    assert orc.orc_rgb_to_yuv(P(rgba), rgba.strides[0], dw, dh, in_order, 1, ctypes.addressof(wp), ctypes.addressof(ws), fmt, 0, wt) == 0
    return want


def expected(orc, src, sw, sh, fmt, interp, order, swap, wt_src, q, fix, yvu_src, l2, amount, lut, wt_sink):
    """the sink planes (Y, U, V or the packed frame) the oracle makes of one track: src = planes()'s (first, second, third plane, strides)"""
    Y, A1, A2, (ys_, s1, s2) = src
    U, V, stri = (A2, A1, (ys_, s2, s1)) if yvu_src else (A1, A2, (ys_, s1, s2))
    rgba = oracle_chain(orc, Y, U, V, stri, sw, sh, interp, order ^ swap, wt_src, q, fix, l2, amount, lut, None)
    return oracle_sink(orc, rgba, sw // 2, sh // 2, fmt, order ^ swap, wt_sink)


def run(gpu, orc, rng, sw, sh, fmt, ntracks=1, interp=3, blend=True, lut=None, order=0, swap=0, wt_src=0, q=2, fix=0, yvu_src=False, pad=(0, 0, 0), tight=False,
        wt_sink=0, yvu_sink=False, pads=(8, 4, 12), srcs=None):
    """one call with ntracks tracks that all differ; the device buffers are allocated in a shuffled order and handed over in another (slot order != frame order); Y, U
    and V planes of the sink have different paddings; every sink plane is compared whole: frame bytes against the oracle, row padding and guard rows against their
    fill.  Returns the expected planes of every track."""
    ops = gpu
    dw, dh = sw // 2, sh // 2
    dims = plane_dims(fmt, dw, dh)
    strides = [align(b + pads[k], 8 if k == 0 else 4) for k, (b, _) in enumerate(dims)]
    irow2 = align(dw * 4, 8) + 24
    srcs = srcs if srcs is not None else [planes(rng, sw, sh, pad, tight) for _ in range(ntracks)]
    l2s = None
    if blend:
        l2s = [rng.integers(0, 256, (dh, irow2), dtype=np.uint8) for _ in range(ntracks)]
        for a in l2s:
            al = a[:, 3:dw * 4:4]
            al[rng.random(al.shape) < 0.5] = 255
    amounts = distinct_amounts(rng, ntracks)
    fills = [[rng.integers(0, 256, (r + GUARD, strides[k]), dtype=np.uint8) for k, (_, r) in enumerate(dims)] for _ in range(ntracks)]
    d_src, d_l2, d_pl = [None] * ntracks, [None] * ntracks, [None] * ntracks
    for i in rng.permutation(ntracks):
        d_pl[i] = [dev(f) for f in fills[i]]
        d_src[i] = [dev(p) for p in srcs[i][:3]]
        d_l2[i] = dev(l2s[i]) if blend else None
    slots = [int(k) for k in rng.permutation(ntracks)]
    # YVU420P: the layer's second plane is V -- the call is handed the planes in Y, U, V order, so on either end buffer 2 travels as U and buffer 1 as V
    ssel = [0, 2, 1] if yvu_src else [0, 1, 2]
    dsel = [0, 2, 1] if (yvu_sink and fmt == YUV420P) else list(range(len(dims)))
    ys_, s1, s2 = srcs[0][3]
    stri = (ys_, s2, s1) if yvu_src else (ys_, s1, s2)
    prm = ops.chain_params(sw, sh, 0, dw, dh, irow2, 0, swap_rb=swap, interp=interp | PIXBUF | (0 if blend else NOBLEND), bf=0, lut=lut)
    src = ops.yuv_source(stri, srcs[0][ssel[1]].size, srcs[0][ssel[2]].size, out_order=order, which_tables=wt_src, pb_quality=q, flags=fix)
    sink = ops.chain_sink(fmt, [strides[j] for j in dsel], which_tables=wt_sink, in_order=order ^ swap)
    trk = ops.chain_yuv_sink_tracks([d_src[k][0] for k in slots], [d_src[k][ssel[1]] for k in slots], [d_src[k][ssel[2]] for k in slots],
                                    [d_l2[k] for k in slots] if blend else None, [[d_pl[k][j] for j in dsel] for k in slots])
    ops.chain_yuv420p_to_yuv(prm, src, sink, trk, [amounts[k] for k in slots] if blend else None)
    wants = []
    for i in range(ntracks):
        want = expected(orc, srcs[i], sw, sh, fmt, interp, order, swap, wt_src, q, fix, yvu_src, l2s[i] if blend else None, amounts[i] if blend else 0, lut, wt_sink)
        wants.append(want)
        for p, j in enumerate(dsel):              # p: the conversion's plane (Y, U, V); j: the buffer it was handed
            b, r = dims[p]
            got = host(d_pl[i][j])
            bad = got[:r, :b] != want[p][:r, :b]
            assert not bad.any(), "track %d plane %d: %d bytes differ from the oracle, first at %s" % (i, p, int(bad.sum()), np.argwhere(bad)[0].tolist())
            assert (got[:r, b:] == fills[i][j][:r, b:]).all(), "track %d plane %d: row padding was written" % (i, p)
            assert (got[r:] == fills[i][j][r:]).all(), "track %d plane %d: guard rows were written" % (i, p)
    return wants


# 520x292 -> 260x146: three strips (both strip parities), dw % 8 == 4 (a half-filled last quad), enough bands for upward-walking ones.  256x144: dw % 8 == 0;
# 264x100: dw % 8 == 4; 256x148: an odd chroma height.  8x4 -> 4x2: a lone half quad, one chroma row, no inner row pair.
MULTI, MID, TINY = (520, 292), [(256, 144), (264, 100), (256, 148)], [(8, 4), (16, 4), (16, 12)]
GEOM = [MULTI] + MID + TINY


def stage_geometries(interp, blend, with_lut, fmt):
    """the three geometries of a stage-matrix case: the multi-strip frame, one tiny frame and one of the middle ones, rotated so that per format the eight stage
    combinations meet all seven geometries (checked below)"""
    c = (interp == 2) * 4 + (not blend) * 2 + (not with_lut) + fmt
    return [MULTI, TINY[c % 3], MID[(c // 2) % 3]]


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [3, 2], ids=["hyper", "bilinear"])
@pytest.mark.parametrize("blend", [True, False], ids=["blend", "noblend"])
@pytest.mark.parametrize("with_lut", [True, False], ids=["lut", "nolut"])
@pytest.mark.parametrize("fmt", [UYVY, YUYV, YUV420P], ids=["uyvy", "yuyv", "yuv420p"])
def test_chain_transcode_stages(gpu, orc, interp, blend, with_lut, fmt):
    """every stage combination to every sink format, each on three geometries (stage_geometries) and with both settings of swap_rb on each; out_order, the source's
    tables, pb_quality, LGPU_YUV_FIX_EDGES and the sink's tables drawn per run, against the oracle"""
    case = ((interp == 2) * 4 + (not blend) * 2 + (not with_lut)) * 3 + (fmt - 2)
    rng = np.random.default_rng(0x7C0DE + case)
    lut = gamma_lut(orc) if with_lut else None
    for i, (sw, sh) in enumerate(stage_geometries(interp, blend, with_lut, fmt)):
        for swap in (0, 1):
            wt_sink = int(rng.integers(0, 4)) if fmt == YUV420P else int(rng.integers(0, 2))
            run(gpu, orc, rng, sw, sh, fmt, ntracks=2, interp=interp, blend=blend, lut=lut, order=int(rng.integers(0, 2)), swap=swap, wt_src=int(rng.integers(0, 4)),
                q=int(rng.integers(1, 4)), fix=int(rng.integers(0, 2)) * FIX_EDGES, yvu_src=bool(i & 1), pad=(3 * i, 5, 1), tight=bool(i), wt_sink=wt_sink,
                yvu_sink=bool(i & 2), pads=(8 * i, 4 + i, 12 - 3 * i))


def test_stage_matrix_covers_every_geometry_for_every_format():
    """the choice above, checked: every case meets the multi-strip frame and a tiny one, and per format all seven geometries of the list are met"""
    for fmt in (UYVY, YUYV, YUV420P):
        seen_fmt = set()
        for interp in (3, 2):
            for blend in (True, False):
                for with_lut in (True, False):
                    g = stage_geometries(interp, blend, with_lut, fmt)
                    assert MULTI in g and any(t in g for t in TINY), (fmt, interp, blend, with_lut, g)
                    seen_fmt.update(g)
        assert seen_fmt == set(GEOM), (fmt, seen_fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("wt", [0, 1, 2, 3])
@pytest.mark.parametrize("q", [1, 2, 3])
@pytest.mark.parametrize("fix", [0, 1])
def test_chain_transcode_source_quirks(gpu, orc, wt, q, fix):
    """the source's four table sets, pb_quality LOW / MED / HIGH, the trailing row with and without LGPU_YUV_FIX_EDGES, through the 4:2:0 sink at 260x146; tight
    chroma planes with odd pitches (K2's read past the last row's end clamped to the plane's last byte)"""
    rng = np.random.default_rng(0x50C + wt * 8 + q * 2 + fix)
    run(gpu, orc, rng, 520, 292, YUV420P, interp=3, blend=True, lut=gamma_lut(orc), wt_src=wt, q=q, fix=fix, pad=(1, 1, 3), tight=True, wt_sink=(wt + q) & 3)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,wt", [(YUV420P, 0), (YUV420P, 1), (YUV420P, 2), (YUV420P, 3), (UYVY, 0), (UYVY, 1), (YUYV, 0), (YUYV, 1)])
def test_chain_transcode_sink_tables(gpu, orc, fmt, wt):
    """every valid table set of every sink format, behind sources of both byte orders"""
    rng = np.random.default_rng(0x51A + fmt * 4 + wt)
    for order in (0, 1):
        run(gpu, orc, rng, 264, 100, fmt, ntracks=2, interp=2, blend=True, order=order, wt_src=wt ^ 1, wt_sink=wt, pad=(0, 2, 6))


def flat_planes(sw, sh, y, u, v):
    """a frame of one colour"""
    hw, hh = sw // 2, sh // 2
    return (np.full((sh, sw), y, np.uint8), np.full(hh * hw, u, np.uint8), np.full(hh * hw, v, np.uint8), (sw, hw, hw))


def test_yuyv_lost_upper_clamp_expectation(orc):
    """the oracle's side of the next test alone: a saturated blue / red frame behind a threshold LUT makes U / V raw 256 with unclamped sink tables, which rgb2yuyv
    (only the lower chroma clamp survives) stores as byte 0 where rgb2uyvy stores 255"""
    lut = np.where(np.arange(256) >= 128, 255, 0).astype(np.uint8)
    for (y, u, v), ch in (((60, 255, 100), 0), ((80, 90, 255), 1)):
        src = flat_planes(48, 12, y, u, v)
        w_yuyv = expected(orc, src, 48, 12, YUYV, 2, 0, 0, 1, 2, 0, False, None, 0, lut, 1)[0]
        w_uyvy = expected(orc, src, 48, 12, UYVY, 2, 0, 0, 1, 2, 0, False, None, 0, lut, 1)[0]
        assert (w_yuyv[:, 1 + 2 * ch::4] == 0).all() and (w_uyvy[:, 2 * ch::4] == 255).all()
        assert (w_yuyv[:, 0::2] == w_uyvy[:, 1::2]).all()          # luma agrees


@pytest.mark.gpu
def test_chain_transcode_yuyv_lost_upper_clamp(gpu, orc):
    """YUYV's missing upper chroma clamp behind the 4:2:0 source (the expectation is shown to carry the quirk by the test above)"""
    rng = np.random.default_rng(0x10C)
    lut = np.where(np.arange(256) >= 128, 255, 0).astype(np.uint8)
    for y, u, v in ((60, 255, 100), (80, 90, 255)):
        src = flat_planes(48, 12, y, u, v)
        for fmt in (YUYV, UYVY):
            run(gpu, orc, rng, 48, 12, fmt, interp=2, blend=False, lut=lut, wt_src=1, wt_sink=1, srcs=[src])


@pytest.mark.gpu
@pytest.mark.parametrize("yvu_src", [False, True], ids=["yuv-in", "yvu-in"])
@pytest.mark.parametrize("yvu_sink", [False, True], ids=["yuv-out", "yvu-out"])
def test_chain_transcode_plane_orders(gpu, orc, yvu_src, yvu_sink):
    """YVU420P on the source, on the sink and on both, by swapped planes; the chroma strides differ on both ends, so a mix-up shows"""
    rng = np.random.default_rng(0x0D + 2 * yvu_src + yvu_sink)
    run(gpu, orc, rng, 264, 100, YUV420P, ntracks=2, interp=3, blend=True, order=1, swap=1, yvu_src=yvu_src, pad=(0, 3, 9), yvu_sink=yvu_sink, pads=(0, 4, 12))


@pytest.mark.gpu
@pytest.mark.parametrize("th", [1, 2, 5, 7])
@pytest.mark.parametrize("sw,sh", [(512, 200), (248, 1000)])
def test_chain_transcode_band_seams_at_forced_heights(gpu, orc, tune, sw, sh, th):
    """the 4:2:0 sink with bands of (about) th rows requested: band boundaries lie at odd rows whatever is asked for, odd bands walk upwards, the carried chroma of a
    row pair's first row and the source's row pairs meet at every seam, and the bytes do not depend on it"""
    tune("PBH_TH", th)
    rng = np.random.default_rng(0xBA5D + sw + th)
    run(gpu, orc, rng, sw, sh, YUV420P, ntracks=2, interp=3, blend=True, lut=gamma_lut(orc), order=th & 1, swap=1, wt_src=th & 3, q=1 + th % 3, fix=th & 1,
        wt_sink=(th >> 1) & 3, pad=(0, 1, 3), tight=True, pads=(0, 8, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("ntracks", [1, 7, 16, 17, 64])
def test_chain_transcode_tracks(gpu, orc, ntracks):
    """1 .. 64 tracks in one call (more than 32 go as two launches) with distinct amounts and shuffled buffers, to every format"""
    rng = np.random.default_rng(0x7AC + ntracks)
    lut = gamma_lut(orc)
    run(gpu, orc, rng, 264, 100, YUV420P, ntracks=ntracks, blend=True, lut=lut, order=1, swap=0, wt_src=2, wt_sink=2, yvu_sink=True, pad=(4, 0, 2), pads=(4, 8, 0))
    run(gpu, orc, rng, 264, 100, UYVY, ntracks=ntracks, blend=True, lut=lut, swap=1, pads=(12, 0, 0))
    run(gpu, orc, rng, 264, 100, YUYV, ntracks=ntracks, interp=2, blend=True, order=1, wt_sink=1, yvu_src=True, pads=(0, 0, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [YUV420P, UYVY], ids=["yuv420p", "uyvy"])
def test_chain_transcode_at_size_matches_two_launches(gpu, fmt):
    """4 x 3840x2160 -> 1920x1080 with blend and gamma (the full-device work order on 256 CUs): byte-identical to the device's own two launches, lgpu_chain_yuv420p
    into an RGBA frame + lgpu_rgb_to_yuv_batch, on the same inputs"""
    import torch
    from oracle import pyoracle
    ops = gpu
    rng = np.random.default_rng(0x51 + fmt)
    sw, sh, dw, dh, n = 3840, 2160, 1920, 1080, 4
    lut = gamma_lut(pyoracle.oracle())
    g = torch.Generator(device="cuda")
    g.manual_seed(8642 + fmt)
    Ys = [torch.randint(0, 256, (sh, sw), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    Us = [torch.randint(0, 256, (sh // 2, sw // 2), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    Vs = [torch.randint(0, 256, (sh // 2, sw // 2), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    L2 = [torch.randint(0, 256, (dh, dw * 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    amounts = [int(x) for x in rng.integers(0, 256, n)]
    dims = plane_dims(fmt, dw, dh)
    fused = [[torch.full((r, b), 0x5C, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
    two = [[torch.full((r, b), 0xC5, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
    prm = ops.chain_params(sw, sh, sw, dw, dh, dw * 4, dw * 4, swap_rb=1, interp=3 | PIXBUF, bf=0, lut=lut)
    src = ops.yuv_source((sw, sw // 2, sw // 2), Us[0].numel(), Vs[0].numel(), out_order=0, which_tables=0, pb_quality=2)
    ops.chain_yuv420p_to_yuv(prm, src, ops.chain_sink(fmt, [b for (b, _) in dims], which_tables=0, in_order=1), ops.chain_yuv_sink_tracks(Ys, Us, Vs, L2, fused), amounts)
    rgba = [torch.zeros((dh, dw * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    ops.chain_yuv420p(prm, src, ops.chain_yuv_tracks(Ys, Us, Vs, L2, rgba), amounts)
    ops.rgb_to_yuv_batch(rgba, two, dw, dh, 1, 1, fmt, 0, 0)
    torch.cuda.synchronize()
    for i in range(n):
        for p in range(len(dims)):
            assert torch.equal(fused[i][p], two[i][p]), "track %d plane %d: %d bytes differ from the two-launch form" % (i, p, int((fused[i][p] != two[i][p]).sum()))


@pytest.mark.gpu
def test_chain_transcode_refusals(gpu):
    """bad arguments -- every one either parent refuses, a sink->in_order that is not the chain's, a destination plane that is a source plane: LGPU_E_BADARG; shapes
    off the one-launch form: LGPU_E_UNSUPPORTED; nothing is written in either case; the same call inside the form runs"""
    import torch
    from lives_amd import lib
    ops = gpu
    sw, sh, dw, dh = 256, 144, 128, 72
    Y = torch.zeros((sh, sw), dtype=torch.uint8, device="cuda")
    U = torch.zeros((sh // 2, sw // 2), dtype=torch.uint8, device="cuda")
    V = torch.zeros_like(U)
    L2 = torch.zeros((dh + 8, dw * 4 + 64), dtype=torch.uint8, device="cuda")
    D = [torch.full((dh + 8, dw * 2 + 64), 0x5C, dtype=torch.uint8, device="cuda") for _ in range(3)]

    def call(fmt=YUV420P, sw_=sw, sh_=sh, dw_=dw, dh_=dh, interp=3 | PIXBUF, blur=0, amounts=(9,), ntracks=1, null_src=False, null_plane=False, strides=(sw, sw // 2, sw // 2),
             usz=None, vsz=None, order=0, swap=0, wt_src=0, q=2, flags=0, wt=0, in_order=None, orow=None, irow2=dw * 4 + 64, dst_off=0, l2_off=0, in_place=None):
        prm = ops.chain_params(sw_, sh_, 0, dw_, dh_, irow2, 0, swap_rb=swap, interp=interp, do_blur=blur, bf=0)
        src = ops.yuv_source(strides, U.numel() if usz is None else usz, V.numel() if vsz is None else vsz, out_order=order, which_tables=wt_src, pb_quality=q, flags=flags)
        sink = ops.chain_sink(fmt, orow if orow is not None else [dw * 2 + 64] * 3, which_tables=wt, in_order=(order ^ swap) if in_order is None else in_order)
        m = max(ntracks, 1)
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
        am = list(amounts) * m if amounts is not None else None
        return ops.chain_yuv420p_to_yuv(prm, src, sink, trk, am, check=False)

    badarg = {
        "no PIXBUF": dict(interp=3),
        "null amounts with a blend": dict(amounts=None),
        "no tracks": dict(ntracks=0),
        "65 tracks": dict(ntracks=65),
        "null source plane": dict(null_src=True),
        "null sink plane": dict(null_plane=True),
        "out_order 2": dict(order=2, in_order=0),
        "source which_tables 4": dict(wt_src=4),
        "pb_quality 0": dict(q=0),
        "unknown flag": dict(flags=2),
        "luma stride below the width": dict(strides=(sw - 4, sw // 2, sw // 2)),
        "chroma stride below the width": dict(strides=(sw, sw // 2 - 2, sw // 2)),
        "chroma plane too small": dict(usz=U.numel() - 1),
        "odd sw": dict(sw_=255, dw_=128),
        "out_fmt 1": dict(fmt=1),
        "out_fmt 6": dict(fmt=6),
        "in_order 2": dict(in_order=2),
        "sink which_tables 4": dict(wt=4),
        "BT.709 with UYVY": dict(fmt=UYVY, wt=2),
        "BT.709 with YUYV": dict(fmt=YUYV, wt=3),
        "odd dw": dict(sw_=254, dw_=127, strides=(254, 127, 127)),
        "sink luma stride below the row": dict(orow=[dw - 8, dw, dw]),
        "sink chroma stride below the row": dict(orow=[dw, dw // 2 - 4, dw]),
        "packed stride below the row": dict(fmt=UYVY, orow=[dw * 2 - 8, 0, 0]),
        "layer-2 stride below the row": dict(irow2=dw * 4 - 8),
        "in_order against the chain's (no swap)": dict(order=1, swap=0, in_order=0),
        "in_order against the chain's (swap)": dict(order=1, swap=1, in_order=1),
        "luma sink plane is the source's luma plane": dict(in_place=(0, 0)),
        "chroma sink plane is a source chroma plane": dict(in_place=(1, 2)),
    }
    unsupported = {
        "not 2:1": dict(sw_=sw - 8),
        "not 2:1 down": dict(sh_=sh - 2),
        "dw % 4 == 2": dict(sw_=252, dw_=126),
        "odd dh with 4:2:0": dict(sh_=142, dh_=71),
        "gaussian": dict(blur=1),
        "nearest": dict(interp=0 | PIXBUF),
        "YUV422P": dict(fmt=5),
        "luma rowstride % 8 != 0": dict(orow=[dw + 4, dw, dw]),
        "chroma rowstride % 4 != 0": dict(orow=[dw + 8, dw // 2 + 2, dw]),
        "packed rowstride % 8 != 0": dict(fmt=YUYV, orow=[dw * 2 + 4, 0, 0]),
        "sink plane not 16-byte aligned": dict(dst_off=8),
        "layer-2 rows not 8-byte aligned": dict(l2_off=4),
    }
    for what, kw in list(badarg.items()) + list(unsupported.items()):
        want = E_UNSUPPORTED if what in unsupported else E_BADARG
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc == want, "%s: %d, expected %d (%s)" % (what, rc, want, lib.load().lgpu_last_error())
        assert all(bool((d == 0x5C).all()) for d in D), "%s: a sink plane was written" % what
        if what in unsupported and what != "gaussian":      # (lgpu_chain_yuv420p has no gaussian either)
            assert b"lgpu_chain_yuv420p + lgpu_rgb_to_yuv_batch" in lib.load().lgpu_last_error(), "%s: the refusal does not name the two-launch form" % what
    assert call(sh_=142, dh_=71, fmt=UYVY) == 0      # any dh for the packed formats
    torch.cuda.synchronize()
    assert not bool((D[0][:71, :dw * 2] == 0x5C).all()) and bool((D[1] == 0x5C).all())
    assert call(order=1, swap=1) == 0                 # and the same call inside the form runs
    torch.cuda.synchronize()
    assert not any(bool((d[:dh // 2, :dw // 2] == 0x5C).all()) for d in D)
