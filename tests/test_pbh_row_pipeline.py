"""k_pb_half's row loop (the walk without the gaussian) prefetches by a compile-time rule: the loop runs while two more rows follow, both of its halves requesting the
next rows without a condition, and a band's last one or two rows are peeled behind it; the band's set-up requests in the loop's own order.  Such a loop can go wrong
at a band's end (the two tail parities, bands too short to enter the loop at all), at the frame's first and last row (clamped source rows), in bands that walk
upwards (odd bands) and where a last band is shorter than the others -- so the frames are small: source 2 dw x 2 dh for

    dw      2 (both frame edges in lane 0), 128 (one whole strip: lane 63's right tap is its own clamped edge load), 130 (a second strip of one lane), 514 (a second
            column group)
    dh      1, 2, 3, 4, 5, 6, 7, 11, 13: frame heights around the band heights
    PBH_TH  unset (the planner: bands of at most 6 rows), 1, 2, 3, 4, 5, 7: bands of 1 to 7 rows -- loop trips 0 to 3, one or two peeled rows -- with odd bands
            walking upwards and, whenever dh is no multiple, bands of two heights

on every form that shares the loop: lgpu_pixbuf_scale at 2:1 with HYPER and with BILINEAR, lgpu_chain with and without swap_rb, LGPU_INTERP_NOBLEND, the feeder-lane
strips (PBH_ALIGNED = 0), lgpu_chain_to_yuv to UYVY and YUV420P (even dh; its widths are multiples of 4).  Everything bit for bit against
tests.chain_ref.oracle_chain_rgba, as tests/test_pbh_row_step.py (whose sources, layer-2 frames and guarded destinations are used here); row padding and guard rows of
every destination must keep their fill.  Last, one launch of 64 tracks with the planner's own bands of two heights."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.chain_ref import Tracks, oracle_chain_rgba
from tests.test_pbh_row_step import Dest, gamma_lut, layer2, sink_planes, source
from tests.util import dev

pytestmark = pytest.mark.gpu
P = po.P
PIXBUF, NOBLEND = 0x100, 0x400
HYPER, BILINEAR = 3, 2
UYVY, YUV420P = 2, 4
WIDTHS = [2, 128, 130, 514]
SINK_WIDTHS = [4, 128, 132, 516]       # lgpu_chain_to_yuv serves dw % 4 == 0 only: the same edge cases at the neighbouring widths
HEIGHTS = [1, 2, 3, 4, 5, 6, 7, 11, 13]
BAND_ROWS = [None, 1, 2, 3, 4, 5, 7]


@pytest.mark.parametrize("dw", WIDTHS)
def test_row_pipeline_rgba_forms(gpu, orc, tune, dw):
    rng = np.random.default_rng(0x13B0 + dw)
    lut = gamma_lut(rng)
    sw = 2 * dw
    for dh in HEIGHTS:
        sh = 2 * dh
        src = source(rng, sw, sh, "random")
        l2 = layer2(rng, dw, dh)
        bf = int(rng.integers(0, 256))
        d_src, d_l2 = dev(src), dev(l2)
        out = Dest(rng, dw * 4, dh)
        irow, irow2, orow = src.strides[0], l2.strides[0], out.fill.strides[0]
        want = {
            "hyper": oracle_chain_rgba(orc, src, sw, sh, dw, dh, HYPER, 0, None, 0, None),
            "bilinear": oracle_chain_rgba(orc, src, sw, sh, dw, dh, BILINEAR, 0, None, 0, None),
            "chain swap": oracle_chain_rgba(orc, src, sw, sh, dw, dh, HYPER, 1, l2, bf, lut),
            "chain": oracle_chain_rgba(orc, src, sw, sh, dw, dh, HYPER, 0, l2, bf, None),
            "chain bilinear": oracle_chain_rgba(orc, src, sw, sh, dw, dh, BILINEAR, 1, l2, bf, lut),
            "noblend": oracle_chain_rgba(orc, src, sw, sh, dw, dh, HYPER, 1, None, 0, lut),
        }
        p_swap = gpu.chain_params(sw, sh, irow, dw, dh, irow2, orow, swap_rb=1, interp=HYPER | PIXBUF, bf=bf, lut=lut)
        p_noswap = gpu.chain_params(sw, sh, irow, dw, dh, irow2, orow, swap_rb=0, interp=HYPER | PIXBUF, bf=bf)
        p_bil = gpu.chain_params(sw, sh, irow, dw, dh, irow2, orow, swap_rb=1, interp=BILINEAR | PIXBUF, bf=bf, lut=lut)
        p_noblend = gpu.chain_params(sw, sh, irow, dw, dh, irow2, orow, swap_rb=1, interp=HYPER | PIXBUF | NOBLEND, bf=0, lut=lut)
        trk, trk_nb = gpu.chain_tracks([d_src], [d_l2], [out.d]), gpu.chain_tracks([d_src], None, [out.d])
        for th in BAND_ROWS:
            tune("PBH_TH", th)
            what = "dw %d dh %d PBH_TH %s" % (dw, dh, th)
            out.reset()
            gpu.pixbuf_scale(d_src, out.d, sw, sh, dw, dh, 4, HYPER)
            out.check(want["hyper"], what + ": lgpu_pixbuf_scale, HYPER")
            out.reset()
            gpu.pixbuf_scale(d_src, out.d, sw, sh, dw, dh, 4, BILINEAR)
            out.check(want["bilinear"], what + ": lgpu_pixbuf_scale, BILINEAR")
            out.reset()
            gpu.chain(p_swap, trk)
            out.check(want["chain swap"], what + ": lgpu_chain, swap_rb")
            out.reset()
            gpu.chain(p_noswap, trk)
            out.check(want["chain"], what + ": lgpu_chain")
            out.reset()
            gpu.chain(p_bil, trk)
            out.check(want["chain bilinear"], what + ": lgpu_chain, BILINEAR, swap_rb")
            out.reset()
            gpu.chain_amounts(p_noblend, trk_nb, None)
            out.check(want["noblend"], what + ": LGPU_INTERP_NOBLEND")
            tune("PBH_ALIGNED", 0)
            out.reset()
            gpu.chain(p_swap, trk)
            out.check(want["chain swap"], what + ": lgpu_chain, swap_rb, PBH_ALIGNED 0")
            out.reset()
            gpu.pixbuf_scale(d_src, out.d, sw, sh, dw, dh, 4, HYPER)
            out.check(want["hyper"], what + ": lgpu_pixbuf_scale, HYPER, PBH_ALIGNED 0")
            tune("PBH_ALIGNED", None)


@pytest.mark.parametrize("fmt", [UYVY, YUV420P], ids=["uyvy", "yuv420p"])
@pytest.mark.parametrize("dw", SINK_WIDTHS)
def test_row_pipeline_yuv_sink(gpu, orc, tune, dw, fmt):
    """lgpu_chain_to_yuv (swap_rb, blend, LUT) at the even heights, every band rule"""
    rng = np.random.default_rng(0x13C0 + dw * 8 + fmt)
    lut = gamma_lut(rng)
    sw = 2 * dw
    for dh in [h for h in HEIGHTS if h % 2 == 0]:
        sh = 2 * dh
        dims = sink_planes(fmt, dw, dh)
        src = source(rng, sw, sh, "random")
        l2 = layer2(rng, dw, dh)
        bf = int(rng.integers(0, 256))
        in_order, wt = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        d_src, d_l2 = dev(src), dev(l2)
        outs = [Dest(rng, b, r, pad=4 + 4 * k) for k, (b, r) in enumerate(dims)]
        rgba = oracle_chain_rgba(orc, src, sw, sh, dw, dh, HYPER, 1, l2, bf, lut)
        want, _ = po.k4_out_planes(0, dw, dh, fmt, 0)
        wp, ws = po.planes_args(want)
        assert orc.orc_rgb_to_yuv(P(rgba), rgba.strides[0], dw, dh, in_order, 1, ctypes.addressof(wp), ctypes.addressof(ws), fmt, 0, wt) == 0
        prm = gpu.chain_params(sw, sh, src.strides[0], dw, dh, l2.strides[0], 0, swap_rb=1, interp=HYPER | PIXBUF, bf=0, lut=lut)
        sink = gpu.chain_sink(fmt, [o.fill.strides[0] for o in outs], which_tables=wt, in_order=in_order)
        trk = gpu.chain_sink_tracks([d_src], [d_l2], [[o.d for o in outs]])
        for th in BAND_ROWS:
            tune("PBH_TH", th)
            for o in outs:
                o.reset()
            gpu.chain_to_yuv(prm, sink, trk, [bf])
            for k, o in enumerate(outs):
                o.check(want[k], "dw %d dh %d PBH_TH %s: plane %d" % (dw, dh, th, k))


def test_row_pipeline_many_tracks_two_band_heights(gpu, orc, tune):
    """64 tracks of 1024x54 -> 512x27 with the planner's own bands: one column group per band, and a band count that does not divide 27, so that the first `rem` bands of
    every track are a row taller than the others (PbHalfArgs.rem) -- the two tail parities side by side in one launch, odd bands upwards.  The library does not report
    the plan of a launch: pb_half_geometry's rule is restated and asserted for this device below (as tests/test_track_counts.py does).  On 256 CUs that is 5 bands of
    6, 6, 5, 5, 5 rows: 320 workgroups, more than one per CU, though fewer than the 8 per CU from which the planner counts a second generation (at this width 64 tracks
    cannot reach that: tests/test_pbh_row_step.py's 64-track case covers that work order with one-row bands).  So the launch is repeated the way the planner shapes one
    of several generations: 8 bands (4, 4, 4, 3, 3, 3, 3, 3 rows), the bands dealt round robin to the XCDs (PBH_ORDER 2), five workgroups per CU (PBH_OCC 5).  Every
    track has its own content, layer 2 and amount (lgpu_chain_amounts), handed over in a shuffled slot order."""
    import torch
    n, dw, dh = 64, 512, 27
    sw, sh = 2 * dw, 2 * dh
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cgroups = ((dw + 127) // 128 + 3) // 4
    bands = (dh + 5) // 6
    if cgroups * n * bands > cus * 8:
        bands = 8 * max(1, (dh + 20) // 40)
    th, rem = dh // bands, dh % bands
    assert cgroups == 1 and rem != 0, "bands of one height only: %d bands of %d rows" % (bands, th)
    assert cgroups * bands * n > cus, "%d workgroups do not outrun %d CUs" % (cgroups * bands * n, cus)
    rng = np.random.default_rng(0x13D5)
    srcs = [source(rng, sw, sh, "random") for i in range(n)]
    T = Tracks(rng, srcs, dw, dh)
    lut = gamma_lut(rng)
    wants = [oracle_chain_rgba(orc, srcs[i], sw, sh, dw, dh, HYPER, 1, T.l2s[i], T.amounts[i], lut) for i in range(n)]
    prm = gpu.chain_params(sw, sh, srcs[0].strides[0], dw, dh, T.irow2, T.orow, swap_rb=1, interp=HYPER | PIXBUF, bf=0, lut=lut)
    gpu.chain_amounts(prm, gpu.chain_tracks(T.slots(T.d_src), T.slots(T.d_l2), T.slots(T.d_dst)), T.slots(T.amounts))
    for i in range(n):
        T.check(i, wants[i], "64 tracks, %d bands of %d / %d rows" % (bands, th + 1, th))
    T.reset()
    tune("PBH_TH", 100000 + 8)
    tune("PBH_ORDER", 2)
    tune("PBH_OCC", 5)
    gpu.chain_amounts(prm, gpu.chain_tracks(T.slots(T.d_src), T.slots(T.d_l2), T.slots(T.d_dst)), T.slots(T.amounts))
    for i in range(n):
        T.check(i, wants[i], "64 tracks, 8 bands of 4 / 3 rows, work order 2")
