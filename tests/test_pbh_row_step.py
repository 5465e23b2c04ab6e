"""The horizontal step of k_pb_half's HYPER form on strips of 64 quads (pb_half_hrow_raw): a lane takes its two foreign pixels per source row -- P[4k-1] from the
left lane, P[4k+4] from the right one, the strip's edge pixel from an extra load in lanes 0 and 63 -- as raw RGBA dwords and premultiplies them itself.  That can
only go wrong at strip edges, frame edges and band seams, so the frames are small: source 2 dw x 2 dh for

    dw   2 (both frame edges in lane 0), 126 (the frame ends in lane 62: lane 63 lies outside), 128 (lane 63's right tap is its own clamped edge load),
         130 (a second strip of one lane, whose left tap is the first strip's last pixel), 258, 512 (one full workgroup), 514 (a second column group)
    dh   1, 2, 7, 14 with the planner's bands and with one-row bands (PBH_TH = 1; odd bands walk upwards)
    alpha  random / all 0 / all 255 / 255 only at source columns 3 mod 4 / 255 only at source columns 0 mod 4 -- in the last two the only pixels with weight at an
         H column's outer tap are the exchanged ones (P[4k-1] and P[4k+4] seen from the neighbouring lane): a wrong neighbour changes every output pixel

on every form that shares the row step: lgpu_pixbuf_scale at 2:1, lgpu_chain with and without swap_rb, LGPU_INTERP_NOBLEND, lgpu_chain_to_yuv to UYVY and YUV420P
(dh even), and the feeder-lane strips (PBH_ALIGNED = 0) as the unchanged twin.  Everything bit for bit against tests.chain_ref.oracle_chain_rgba; row padding and
guard rows of every destination must keep their fill.  Last, the full-device path at small size: 64 tracks, 2560 workgroups."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.chain_ref import Tracks, oracle_chain_rgba
from tests.util import align, dev, host

pytestmark = pytest.mark.gpu
P = po.P
PIXBUF, NOBLEND = 0x100, 0x400
E_UNSUPPORTED = -3
UYVY, YUV420P = 2, 4
GUARD = 2
WIDTHS = [2, 126, 128, 130, 258, 512, 514]
# lgpu_chain_to_yuv serves dw % 4 == 0 only: the widths above that it takes, and their neighbours with the same edge cases -- 4 (both frame edges in lanes 0 and 1),
# 124 (the frame ends in lane 61), 132 (a second strip of two lanes), 260, 516 (a second column group)
SINK_WIDTHS = [4, 124, 128, 132, 260, 512, 516]
HEIGHTS = [1, 2, 7, 14]
ALPHAS = ["random", "zero", "opaque", "col3", "col0"]


def source(rng, sw, sh, alpha):
    """random colours, row padding of random bytes (a tap read beyond the row's last pixel shows), the alpha pattern of the case"""
    src = rng.integers(0, 256, (sh, align(sw * 4, 16) + 16), dtype=np.uint8)
    al = src[:, 3:sw * 4:4]
    if alpha == "zero":
        al[:] = 0
    elif alpha == "opaque":
        al[:] = 255
    elif alpha in ("col3", "col0"):
        al[:] = 0
        al[:, (3 if alpha == "col3" else 0)::4] = 255
    return src


def layer2(rng, dw, dh):
    l2 = rng.integers(0, 256, (dh, align(dw * 4, 8) + 24), dtype=np.uint8)
    al = l2[:, 3:dw * 4:4]
    al[rng.random(al.shape) < 0.5] = 255
    return l2


class Dest:
    """a destination with row padding and guard rows of random fill"""

    def __init__(self, rng, row_bytes, rows, pad=8):
        self.b, self.r = row_bytes, rows
        self.fill = rng.integers(0, 256, (rows + GUARD, align(row_bytes + pad, 8)), dtype=np.uint8)
        self.d = dev(self.fill)

    def reset(self):
        self.d.copy_(dev(self.fill))

    def check(self, want, what):
        got = host(self.d)
        bad = got[:self.r, :self.b] != want[:self.r, :self.b]
        assert not bad.any(), "%s: %d bytes differ from the oracle, first at %s" % (what, int(bad.sum()), np.argwhere(bad)[0].tolist())
        assert (got[:self.r, self.b:] == self.fill[:self.r, self.b:]).all(), what + ": row padding was written"
        assert (got[self.r:] == self.fill[self.r:]).all(), what + ": guard rows were written"


def gamma_lut(rng):
    return rng.permutation(256).astype(np.uint8)


@pytest.mark.parametrize("dw", WIDTHS)
def test_row_step_rgba_forms(gpu, orc, tune, dw):
    """lgpu_pixbuf_scale at 2:1, lgpu_chain with and without swap_rb, LGPU_INTERP_NOBLEND: every height, alpha pattern and band rule; the chain with swap_rb also on
    the feeder-lane strips"""
    rng = np.random.default_rng(0x7B0 + dw)
    lut = gamma_lut(rng)
    sw = 2 * dw
    for dh in HEIGHTS:
        sh = 2 * dh
        for alpha in ALPHAS:
            src = source(rng, sw, sh, alpha)
            l2 = layer2(rng, dw, dh)
            bf = int(rng.integers(0, 256))
            d_src, d_l2 = dev(src), dev(l2)
            out = Dest(rng, dw * 4, dh)
            irow, irow2, orow = src.strides[0], l2.strides[0], out.fill.strides[0]
            want = {
                "scale": oracle_chain_rgba(orc, src, sw, sh, dw, dh, 3, 0, None, 0, None),
                "chain swap": oracle_chain_rgba(orc, src, sw, sh, dw, dh, 3, 1, l2, bf, lut),
                "chain": oracle_chain_rgba(orc, src, sw, sh, dw, dh, 3, 0, l2, bf, None),
                "noblend": oracle_chain_rgba(orc, src, sw, sh, dw, dh, 3, 1, None, 0, lut),
            }
            p_swap = gpu.chain_params(sw, sh, irow, dw, dh, irow2, orow, swap_rb=1, interp=3 | PIXBUF, bf=bf, lut=lut)
            p_noswap = gpu.chain_params(sw, sh, irow, dw, dh, irow2, orow, swap_rb=0, interp=3 | PIXBUF, bf=bf)
            p_noblend = gpu.chain_params(sw, sh, irow, dw, dh, irow2, orow, swap_rb=1, interp=3 | PIXBUF | NOBLEND, bf=0, lut=lut)
            trk, trk_nb = gpu.chain_tracks([d_src], [d_l2], [out.d]), gpu.chain_tracks([d_src], None, [out.d])
            for th in (None, 1):
                tune("PBH_TH", th)
                what = "dw %d dh %d alpha %s PBH_TH %s" % (dw, dh, alpha, th)
                out.reset()
                gpu.pixbuf_scale(d_src, out.d, sw, sh, dw, dh, 4, 3)
                out.check(want["scale"], what + ": lgpu_pixbuf_scale")
                out.reset()
                gpu.chain(p_swap, trk)
                out.check(want["chain swap"], what + ": lgpu_chain, swap_rb")
                out.reset()
                gpu.chain(p_noswap, trk)
                out.check(want["chain"], what + ": lgpu_chain")
                out.reset()
                gpu.chain_amounts(p_noblend, trk_nb, None)
                out.check(want["noblend"], what + ": LGPU_INTERP_NOBLEND")
                tune("PBH_ALIGNED", 0)
                out.reset()
                gpu.chain(p_swap, trk)
                out.check(want["chain swap"], what + ": lgpu_chain, swap_rb, PBH_ALIGNED 0")
                tune("PBH_ALIGNED", None)


def sink_planes(fmt, dw, dh):
    return [(dw * 2, dh)] if fmt == UYVY else [(dw, dh), (dw >> 1, dh >> 1), (dw >> 1, dh >> 1)]


@pytest.mark.parametrize("fmt", [UYVY, YUV420P], ids=["uyvy", "yuv420p"])
@pytest.mark.parametrize("dw", SINK_WIDTHS)
def test_row_step_yuv_sink(gpu, orc, tune, dw, fmt):
    """lgpu_chain_to_yuv (swap_rb, blend, LUT) at even heights, every alpha pattern and band rule"""
    rng = np.random.default_rng(0x51B0 + dw * 8 + fmt)
    lut = gamma_lut(rng)
    sw = 2 * dw
    for dh in [h for h in HEIGHTS if h % 2 == 0]:
        sh = 2 * dh
        dims = sink_planes(fmt, dw, dh)
        for alpha in ALPHAS:
            src = source(rng, sw, sh, alpha)
            l2 = layer2(rng, dw, dh)
            bf = int(rng.integers(0, 256))
            in_order, wt = int(rng.integers(0, 2)), int(rng.integers(0, 2))
            d_src, d_l2 = dev(src), dev(l2)
            outs = [Dest(rng, b, r, pad=4 + 4 * k) for k, (b, r) in enumerate(dims)]
            rgba = oracle_chain_rgba(orc, src, sw, sh, dw, dh, 3, 1, l2, bf, lut)
            want, _ = po.k4_out_planes(0, dw, dh, fmt, 0)
            wp, ws = po.planes_args(want)
            assert orc.orc_rgb_to_yuv(P(rgba), rgba.strides[0], dw, dh, in_order, 1, ctypes.addressof(wp), ctypes.addressof(ws), fmt, 0, wt) == 0
            prm = gpu.chain_params(sw, sh, src.strides[0], dw, dh, l2.strides[0], 0, swap_rb=1, interp=3 | PIXBUF, bf=0, lut=lut)
            sink = gpu.chain_sink(fmt, [o.fill.strides[0] for o in outs], which_tables=wt, in_order=in_order)
            trk = gpu.chain_sink_tracks([d_src], [d_l2], [[o.d for o in outs]])
            for th in (None, 1):
                tune("PBH_TH", th)
                for o in outs:
                    o.reset()
                gpu.chain_to_yuv(prm, sink, trk, [bf])
                for k, o in enumerate(outs):
                    o.check(want[k], "dw %d dh %d alpha %s PBH_TH %s: plane %d" % (dw, dh, alpha, th, k))


@pytest.mark.parametrize("dw", [w for w in WIDTHS if w % 4])
def test_yuv_sink_refuses_widths_off_four(gpu, dw):
    """the widths of the RGBA cases that the sink form does not serve (dw % 4 == 2) are refused, not run some other way: nothing is written"""
    import torch
    dh = 2
    src = torch.zeros((2 * dh, align(2 * dw * 4, 16)), dtype=torch.uint8, device="cuda")
    l2 = torch.zeros((dh, align(dw * 4, 8)), dtype=torch.uint8, device="cuda")
    out = torch.full((dh + GUARD, align(dw * 2, 8) + 8), 0x5C, dtype=torch.uint8, device="cuda")
    prm = gpu.chain_params(2 * dw, 2 * dh, src.stride(0), dw, dh, l2.stride(0), 0, swap_rb=1, interp=3 | PIXBUF, bf=0)
    rc = gpu.chain_to_yuv(prm, gpu.chain_sink(UYVY, [out.stride(0)]), gpu.chain_sink_tracks([src], [l2], [[out]]), [7], check=False)
    torch.cuda.synchronize()
    assert rc == E_UNSUPPORTED, rc
    assert bool((out == 0x5C).all())


def test_row_step_full_device_small(gpu, orc, tune):
    """64 tracks of 260x80 -> 130x40 with one-row bands: 64 x 40 workgroups, more than eight per CU, so the launch takes work order 2 and five workgroups per CU;
    every track its own content (alpha patterns in turn), layer 2 and amount (lgpu_chain_amounts), handed over in a shuffled slot order.  The library does not
    report the plan of a launch: work order and occupancy are inferred from pb_chain_half's rule (column groups x bands x tracks > CUs x 8), restated and asserted
    for this device below, as tests/test_track_counts.py does"""
    import torch
    n, dw, dh = 64, 130, 40
    sw, sh = 2 * dw, 2 * dh
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cgroups, bands = ((dw + 127) // 128 + 3) // 4, dh        # two strips of 128 columns = one column group; PBH_TH 1: a band per row
    assert cgroups == 1 and cgroups * bands * n > cus * 8, "%d workgroups do not outrun %d CUs x 8" % (cgroups * bands * n, cus)
    rng = np.random.default_rng(0xF0D5)
    srcs = [source(rng, sw, sh, ALPHAS[i % len(ALPHAS)]) for i in range(n)]
    T = Tracks(rng, srcs, dw, dh)
    lut = gamma_lut(rng)
    wants = [oracle_chain_rgba(orc, srcs[i], sw, sh, dw, dh, 3, 1, T.l2s[i], T.amounts[i], lut) for i in range(n)]
    prm = gpu.chain_params(sw, sh, srcs[0].strides[0], dw, dh, T.irow2, T.orow, swap_rb=1, interp=3 | PIXBUF, bf=0, lut=lut)
    tune("PBH_TH", 1)
    gpu.chain_amounts(prm, gpu.chain_tracks(T.slots(T.d_src), T.slots(T.d_l2), T.slots(T.d_dst)), T.slots(T.amounts))
    for i in range(n):
        T.check(i, wants[i], "64 tracks, PBH_TH 1")
