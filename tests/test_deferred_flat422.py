"""lives_gpu_set_flat_yuv(1) and 4:2:2 sources: convert_layer_palette of a pinned YUV422P / UYVY / YUYV layer to RGBA32 / BGRA32 is recorded as the program's first stage,
and a flush runs a group that keeps its size as ONE lgpu_chain_flat_yuv422 launch -- no conversion pre-launch, no RGBA frame -- with or without a YUV sink behind it.  A
scaled group takes the batched conversion and the RGBA paths (the 2:1 YUV chains are 4:2:0 only and must never see these planes).  With the switch off nothing is
recorded for these palettes.  Compared three ways, as tests/test_deferred_flat.py does: deferred == eager (lives_gpu_set_deferred(0)) == the oracle's composition,
leaves included."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.test_deferred import LEAVES, deferred, oracle_step, plan_step, seam, srgb_to, view  # noqa: F401 (fixtures)
from tests.test_deferred_flat import NSTATS, delta, flat, stats  # noqa: F401 (fixture)
from tests.test_deferred_transcode import K4_FMT, equal_states, same_planes, state, tick_calls
from tests.util import frame

needs_ref = pytest.mark.skipif(not po.have_ref(), reason="oracle/_ref (reference libweed) not built")
pytestmark = [needs_ref, pytest.mark.gpu]
P = po.P
RGBA32, BGRA32, YUV420P, YVU420P, YUV422P, UYVY, YUYV = 3, 4, 512, 513, 522, 564, 565
CLAMPED, UNCLAMPED, SUBSPACE_YCBCR = 0, 1, 1
SRC_PALS = [YUV422P, UYVY, YUYV]
SRC_IDS = ["yuv422p", "uyvy", "yuyv"]


def src_planes(rng, pal, w, h):
    """a w x h frame of `pal` with padded rows (packed rows keep a multiple of 4)"""
    if pal == YUV422P:
        return [rng.integers(0, 256, (h, w + 4), dtype=np.uint8), rng.integers(0, 256, (h, w // 2 + 2), dtype=np.uint8), rng.integers(0, 256, (h, w // 2 + 6), dtype=np.uint8)]
    return [rng.integers(0, 256, (h, w * 2 + 8), dtype=np.uint8)]


def src_layer(wh, pal, w, h, planes):
    """a packed layer's width leaf counts macropixels"""
    return wh.new_layer(pal, w if pal == YUV422P else w // 2, h, planes, gamma=1, clamping=CLAMPED, subspace=SUBSPACE_YCBCR)


def oracle_conv(orc, pal, planes, w, h, order):
    rgba = np.zeros((h, w * 4), np.uint8)
    if pal == YUV422P:
        Y, U, V = planes
        st = (ctypes.c_int * 3)(Y.strides[0], U.strides[0], V.strides[0])
        orc.orc_yuv420p_to_rgb(P(Y), P(U), P(V), st, U.size, V.size, P(rgba), w * 4, w, h, 4, order, 1, 0, 2, None, 0)
    else:
        sp, ss = po.planes_args(planes)
        assert orc.orc_yuv_to_rgb(ctypes.addressof(sp), ctypes.addressof(ss), w, h, 2 if pal == UYVY else 3, 0, P(rgba), w * 4, order, 1, 0) == 0
    return rgba


def oracle_rgba(orc, pal, planes, sw, sh, l2, dw, dh, canvas, bf, lut):
    return oracle_step(orc, oracle_conv(orc, pal, planes, sw, sh, 0), sw, sh, l2, dw, dh, canvas, bf, lut, False)


def oracle_sink(orc, pal, planes, sw, sh, mid, l2, dw, dh, bf, lut, outpl, clamping):
    order = 1 if mid == BGRA32 else 0
    out = oracle_step(orc, oracle_conv(orc, pal, planes, sw, sh, order), sw, sh, l2, dw, dh, None, bf, lut, False)
    fmt = K4_FMT[outpl]
    w, h = (dw & ~1, dh & ~1) if fmt == 4 else (dw, dh)
    want, _ = po.k4_out_planes(0, w, h, fmt, 0)
    wp, ws = po.planes_args(want)
    assert orc.orc_rgb_to_yuv(P(out), out.strides[0], w, h, order, 1, ctypes.addressof(wp), ctypes.addressof(ws), fmt, 0, 1 if clamping == UNCLAMPED else 0) == 0
    return [want[0], want[2], want[1]] if outpl == YVU420P else want


def rgba_group(L, wh, H, orc, pal, sw, sh, dw, dh, canvas, n, seed):
    """n tracks of one shape from `pal` layers, deferred and eager: (counter deltas of the deferred run, of the eager run, results[mode][track], oracle bytes per track)"""
    rng = np.random.default_rng(seed)
    ow, oh = canvas if canvas else (dw, dh)
    srcs = [src_planes(rng, pal, sw, sh) for _ in range(n)]
    l2s = [frame(rng, ow, oh, 4, alpha_mix=True) for _ in range(n)]
    results, ds = [], []
    try:
        for mode in (1, 0):
            L.lives_gpu_set_deferred(mode)
            lays = [src_layer(wh, pal, sw, sh, srcs[i]) for i in range(n)]
            l2l = [wh.new_layer(RGBA32, ow, oh, [a], gamma=1) for a in l2s]
            for a in lays + l2l:
                assert L.lives_gpu_layer_pin(a) == 0
            s0 = stats(L)
            for i in range(n):
                plan_step(L, wh, H, lays[i], l2l[i], dw, dh, canvas, 40 + 13 * i, 2)
            assert L.lives_gpu_layers_flush((ctypes.c_void_p * n)(*lays), n) == 0
            ds.append(delta(s0, stats(L)))
            out = []
            for i in range(n):
                assert L.lives_gpu_layer_sync(lays[i]) == 0
                out.append(([wh.geti(lays[i], k) for k in LEAVES] + [wh.planes_of(lays[i])[2]], view(wh, lays[i])[:, :ow * 4].copy()))
            results.append(out)
            for a in lays + l2l:
                assert L.lives_gpu_layer_unpin(a) == 0
    finally:
        L.lives_gpu_set_deferred(1)
    assert ds[1] == [0] * NSTATS, "the eager run records and launches nothing deferred: %s" % ds[1]
    lut = srgb_to(orc, 2)
    wants = [oracle_rgba(orc, pal, srcs[i], sw, sh, l2s[i], dw, dh, canvas, 40 + 13 * i, lut) for i in range(n)]
    return ds[0], results, wants


def check_rgba(results, wants):
    for i, want in enumerate(wants):
        assert results[0][i][0] == results[1][i][0], "leaves, track %d: %s / %s" % (i, results[0][i][0], results[1][i][0])
        assert (results[0][i][1] == results[1][i][1]).all(), "deferred == eager, track %d" % i
        assert (results[0][i][1] == want).all(), "deferred == oracle, track %d" % i


def sink_group(L, wh, H, orc, pal, sw, sh, dw, dh, outpl, mid, clamping, n, seed):
    """n tracks (blend, gamma) from `pal` layers that end in the sink palette, deferred and eager; returns the deferred run's counter deltas"""
    rng = np.random.default_rng(seed)
    srcs = [src_planes(rng, pal, sw, sh) for _ in range(n)]
    l2s = [frame(rng, dw, dh, 4, alpha_mix=True) for _ in range(n)]
    results, d = [], None
    try:
        for mode in (1, 0):
            L.lives_gpu_set_deferred(mode)
            lays = [src_layer(wh, pal, sw, sh, srcs[i]) for i in range(n)]
            l2l = [wh.new_layer(mid, dw, dh, [a], gamma=1) for a in l2s]
            for a in lays + l2l:
                assert L.lives_gpu_layer_pin(a) == 0
            s0 = stats(L)
            for i in range(n):
                tick_calls(L, wh, H, lays[i], l2l[i], mid, dw, dh, None, 40 + 13 * i, outpl, clamping)
            assert L.lives_gpu_layers_flush((ctypes.c_void_p * n)(*lays), n) == 0
            dd = delta(s0, stats(L))
            if mode:
                d = dd
            else:
                assert dd == [0] * NSTATS
            out = []
            for i in range(n):
                assert L.lives_gpu_layer_sync(lays[i]) == 0
                out.append(state(wh, lays[i]))
            assert delta(s0, stats(L)) == dd, "the syncs ran nothing more"
            results.append(out)
            for a in lays + l2l:
                assert L.lives_gpu_layer_unpin(a) == 0
    finally:
        L.lives_gpu_set_deferred(1)
    lut = srgb_to(orc, 2)
    for i in range(n):
        equal_states(results[0][i], results[1][i], "track %d deferred / eager" % i)
        want = oracle_sink(orc, pal, srcs[i], sw, sh, mid, l2s[i], dw, dh, 40 + 13 * i, lut, outpl, clamping)
        same_planes(results[0][i][1], want, "track %d deferred / oracle" % i)
    return d


SHAPES = [(None, "no resize"), ((160, 100), "letterbox")]


@pytest.mark.parametrize("n", [1, 3, 16])
@pytest.mark.parametrize("canvas", [s[0] for s in SHAPES], ids=[s[1] for s in SHAPES])
@pytest.mark.parametrize("pal", SRC_PALS, ids=SRC_IDS)
def test_flat422_rgba_tick_is_one_launch(seam, orc, deferred, flat, pal, canvas, n):
    """convert_layer_palette -> [letterbox] -> chroma blend -> gamma with the route on: every conversion recorded [4], ONE chain launch [1] carrying n tracks [2], which
    is the flat launch [13] / [14]; no conversion pre-launch [7], no 2:1 YUV launch [5], nothing staged [3]; bytes and leaves equal across deferred, eager and the oracle"""
    L, wh, H = seam
    assert flat(1) == 0
    d, results, wants = rgba_group(L, wh, H, orc, pal, 128, 72, 128, 72, canvas, n, 0x422 + pal + n + (canvas[0] if canvas else 0))
    assert d[4] == n, "every conversion was recorded: %s" % d
    assert (d[1], d[2], d[3], d[5], d[7], d[13], d[14]) == (1, n, 0, 0, 0, 1, n), "one lgpu_chain_flat_yuv422 launch with %d tracks: %s" % (n, d)
    check_rgba(results, wants)


SINK_CASES = [(UYVY, RGBA32, CLAMPED), (YUV420P, BGRA32, CLAMPED), (YVU420P, RGBA32, UNCLAMPED), (YUYV, BGRA32, UNCLAMPED)]


@pytest.mark.parametrize("n", [1, 3, 16])
@pytest.mark.parametrize("outpl,mid,clamping", SINK_CASES, ids=["to_uyvy", "to_yuv420p", "to_yvu420p", "to_yuyv"])
@pytest.mark.parametrize("pal", SRC_PALS, ids=SRC_IDS)
def test_flat422_sink_tick_is_one_launch(seam, orc, deferred, flat, pal, outpl, mid, clamping, n):
    """the same tick followed by the sink conversion with the route on: ONE launch which is the chain launch [1], the sink launch [9], fused [11] and flat [13],
    carrying n tracks; no conversion pre-launch [7], not the 2:1 forms [5] / [12]; planes and leaves equal across deferred, eager and the oracle"""
    L, wh, H = seam
    assert flat(1) == 0
    d = sink_group(L, wh, H, orc, pal, 128, 72, 128, 72, outpl, mid, clamping, n, 0x4225 + pal + outpl + n)
    assert (d[4], d[8]) == (n, n), "every conversion was recorded, at both ends: %s" % d
    assert (d[1], d[9], d[11], d[13]) == (1, 1, 1, 1) and (d[2], d[10], d[14]) == (n, n, n), "ONE lgpu_chain_flat_yuv422 launch with %d tracks: %s" % (n, d)
    assert (d[3], d[5], d[7], d[12]) == (0, 0, 0, 0), d


@pytest.mark.parametrize("pal", SRC_PALS, ids=SRC_IDS)
def test_scaled_group_takes_the_batched_conversion(seam, orc, deferred, flat, pal):
    """an exact 2:1 group with the route on: the 2:1 YUV chains are 4:2:0 only, so the group converts in one batch [7] and scales as the RGBA chain [1]; [5], [12] and
    [13] do not advance; to RGBA and to a UYVY sink; the same bytes as the eager run and the oracle"""
    L, wh, H = seam
    assert flat(1) == 0
    n = 3
    d, results, wants = rgba_group(L, wh, H, orc, pal, 256, 144, 128, 72, None, n, 0x4229 + pal)
    assert d[4] == n and (d[1], d[2], d[3], d[5], d[7], d[13], d[14]) == (1, n, 0, 0, 1, 0, 0), d
    check_rgba(results, wants)
    d = sink_group(L, wh, H, orc, pal, 256, 144, 128, 72, UYVY, RGBA32, CLAMPED, n, 0x422A + pal)
    assert (d[4], d[8]) == (n, n) and (d[3], d[5], d[7], d[12], d[13], d[14]) == (0, 0, 1, 0, 0, 0), d


@pytest.mark.parametrize("pal", SRC_PALS, ids=SRC_IDS)
def test_route_off_records_nothing_for_these_palettes(seam, orc, deferred, flat, pal):
    """with the setter at 0 (the default) the conversion of these palettes runs when it is called, and EVERY counter is what a tick from an RGBA frame gives: no
    conversion recorded [4], no YUV launch of any kind ([5], [6], [7], [12], [13], [14]); the stages behind it are recorded on the RGBA frame and run as the RGBA chain"""
    L, wh, H = seam
    n = 3
    for canvas, _ in SHAPES:
        d, results, wants = rgba_group(L, wh, H, orc, pal, 128, 72, 128, 72, canvas, n, 0x422C + pal)
        print("switch off, pal %d, canvas %s: %s" % (pal, canvas, d))
        # what a tick from a RESIDENT RGBA frame gives (the conversion has run when the next call comes): a letterbox, a blend or a table is recorded only onto a
        # plane that is already a pending program (letterbox_layer, lives_gpu_deferred_blend_chroma and gamma_convert_sub_layer all ask plane_is_lazy / Dev::lazy), and
        # a resize to the same size returns at once.  Nothing starts a program, with or without the letterbox: every call runs its own kernel and every counter stays
        assert d == [0] * NSTATS, d
        check_rgba(results, wants)
    d = sink_group(L, wh, H, orc, pal, 128, 72, 128, 72, YUV420P, RGBA32, CLAMPED, n, 0x422D + pal)
    print("switch off, pal %d, sink: %s" % (pal, d))
    # no letterbox: blend and table run when called (above); the sink conversion of the resident frame is recorded per track [0] / [8] and the flush runs the programs of
    # the sink stage alone as ONE batched conversion [9] of n tracks [10], not fused [11]; no chain launch, nothing else
    assert d == [n, 0, 0, 0, 0, 0, 0, 0, n, 1, n, 0, 0, 0, 0], d


def test_seam_staged_wins_over_the_422_route(seam, orc, deferred, flat, tune):
    """SEAM_STAGED with the route on: no flat launch, no chain launch, one conversion per track and every program walked stage by stage, the oracle's bytes"""
    L, wh, H = seam
    assert flat(1) == 0
    tune("SEAM_STAGED", 1)
    n = 3
    for pal in SRC_PALS:
        d, results, wants = rgba_group(L, wh, H, orc, pal, 128, 72, 128, 72, (160, 100), n, 0x422E + pal)
        assert (d[1], d[3], d[5], d[7], d[13], d[14]) == (0, n, 0, 0, 0, 0), d
        check_rgba(results, wants)
