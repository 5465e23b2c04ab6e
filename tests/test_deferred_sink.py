"""Deferred execution of a tick's LAST call on pinned layers: convert_layer_palette[_full](RGBA32 / BGRA32 -> YUV420P / YVU420P / UYVY / YUYV) -- the hand-over to a
playback plugin or an encoder, src/player.c:1364 -- is recorded as the last stage of the track's program (LZ_SINK, include/lives_gpu_layer.h) and a flush runs the
tick's programs of one shape as ONE lgpu_chain_to_yuv launch in the exact 2:1 shape, as the chain group followed by one lgpu_rgb_to_yuv_batch otherwise, and programs
of the sink stage alone as one lgpu_rgb_to_yuv_batch.  Compared three ways, as tests/test_deferred.py does: deferred == eager (lives_gpu_set_deferred(0)) == the
oracle's composition ... -> orc_rgb_to_yuv, on every plane and on the layer's leaves."""
import ctypes
import threading

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.test_deferred import deferred, oracle_step, plan_step, seam, srgb_to  # noqa: F401 (fixtures)
from tests.util import frame

needs_ref = pytest.mark.skipif(not po.have_ref(), reason="oracle/_ref (reference libweed) not built")
pytestmark = [needs_ref, pytest.mark.gpu]
P = po.P
RGBA32, BGRA32, ARGB32, YUV420P, YVU420P, UYVY, YUYV, A8 = 3, 4, 7, 512, 513, 564, 565, 1024
K4_FMT = {YUV420P: 4, YVU420P: 4, UYVY: 2, YUYV: 3}
CLAMPED, UNCLAMPED = 0, 1
SINK_LEAVES = ("current_palette", "width", "height", "YUV_clamping", "YUV_subspace", "YUV_sampling", "gamma_type", "host_flags")
SINKS = [YUV420P, YVU420P, UYVY, YUYV]


def stats(L):
    L.lives_gpu_deferred_stats_n.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    L.lives_gpu_deferred_stats_n.restype = None
    a = (ctypes.c_ulonglong * 12)()
    L.lives_gpu_deferred_stats_n(a, 12)
    return list(a)


def delta(a, b):
    return [y - x for x, y in zip(a, b)]


def oracle_sink(orc, rgba, w, h, order, outpl, clamping):
    """K4 on an RGBA / BGRA frame into compact planes, in the LAYER's plane order (YVU420P stores V second); 4:2:0 truncates to even sides"""
    fmt = K4_FMT[outpl]
    if fmt == 4:
        w, h = w & ~1, h & ~1
    want, _ = po.k4_out_planes(0, w, h, fmt, 0)
    wp, ws = po.planes_args(want)
    assert orc.orc_rgb_to_yuv(P(rgba), rgba.strides[0], w, h, order, 1, ctypes.addressof(wp), ctypes.addressof(ws), fmt, 0, 1 if clamping == UNCLAMPED else 0) == 0
    return [want[0], want[2], want[1]] if outpl == YVU420P else want


def state(wh, lay):
    """the layer's leaves (rowstrides among them) and copies of its planes"""
    planes, _, rs = wh.planes_of(lay)
    return [wh.geti(lay, k) for k in SINK_LEAVES] + [rs], planes


def same_planes(got, want, what=""):
    assert len(got) == len(want), what
    for p, (g, x) in enumerate(zip(got, want)):
        r, b = x.shape
        assert g.shape[0] == r and (g[:, :b] == x).all(), "%s plane %d differs" % (what, p)


def equal_states(a, b, what=""):
    assert a[0] == b[0], "%s leaves: %s / %s" % (what, a[0], b[0])
    assert len(a[1]) == len(b[1]) and all((x == y).all() for x, y in zip(a[1], b[1])), "%s planes (row padding included)" % what


@pytest.mark.parametrize("outpl", SINKS, ids=["yuv420p", "yvu420p", "uyvy", "yuyv"])
@pytest.mark.parametrize("inpl", [RGBA32, BGRA32], ids=["rgba", "bgra"])
@pytest.mark.parametrize("clamping", [CLAMPED, UNCLAMPED], ids=["clamped", "unclamped"])
def test_sink_alone_deferred_equals_eager_equals_oracle(seam, orc, deferred, outpl, inpl, clamping):
    """the conversion on a pinned layer with no pending program: recorded as a program of the sink stage alone; planes and leaves equal across the three"""
    L, wh, H = seam
    w, h = 136, 74
    rng = np.random.default_rng(outpl * 8 + inpl * 2 + clamping)
    src = frame(rng, w, h, 4, alpha_mix=True)
    out = []
    for mode in (1, 0):
        L.lives_gpu_set_deferred(mode)
        lay = wh.new_layer(inpl, w, h, [src], gamma=1)
        assert L.lives_gpu_layer_pin(lay) == 0
        s0 = stats(L)
        assert L.lives_gpu_convert_layer_palette(lay, outpl, clamping) == 1
        d = delta(s0, stats(L))
        assert (d[8], d[9]) == ((1, 0) if mode else (0, 0)), d
        assert L.lives_gpu_layer_sync(lay) == 0
        d = delta(s0, stats(L))
        assert (d[9], d[10], d[11], d[1], d[3]) == ((1, 1, 0, 0, 0) if mode else (0, 0, 0, 0, 0)), d
        out.append(state(wh, lay))
        assert L.lives_gpu_layer_unpin(lay) == 0
    L.lives_gpu_set_deferred(1)
    equal_states(out[0], out[1], "deferred / eager")
    same_planes(out[0][1], oracle_sink(orc, src, w, h, 1 if inpl == BGRA32 else 0, outpl, clamping), "deferred / oracle")
    lw = w >> 1 if outpl in (UYVY, YUYV) else w
    assert out[0][0][:7] == [outpl, lw, h, clamping, 1, 0, 1]            # YCbCr subspace, default sampling, the gamma as it was


@pytest.mark.parametrize("outpl", SINKS, ids=["yuv420p", "yvu420p", "uyvy", "yuyv"])
def test_sixteen_track_tick_ends_at_the_sink_in_one_launch(seam, orc, deferred, outpl):
    """16 pinned BGRA32 tracks, one host thread per track: convert -> resize 2:1 -> chroma blend -> gamma -> conversion to the sink's palette, one flush: 16 sink stages
    recorded, ONE chain launch carrying 16 tracks which is the ONE sink launch, nothing staged; planes and leaves equal across deferred, eager and the oracle"""
    L, wh, H = seam
    rng = np.random.default_rng(0x51D0 + outpl)
    sw, sh, dw, dh, n = 256, 144, 128, 72, 16
    srcs = [frame(rng, sw, sh, 4, alpha_mix=True) for _ in range(n)]
    l2s = [frame(rng, dw, dh, 4, alpha_mix=True) for _ in range(n)]
    clamping = UNCLAMPED if outpl in (YVU420P, YUYV) else CLAMPED
    results = []
    for mode in (1, 0):
        L.lives_gpu_set_deferred(mode)
        lays = [wh.new_layer(BGRA32, sw, sh, [s], gamma=1) for s in srcs]
        l2l = [wh.new_layer(RGBA32, dw, dh, [a], gamma=1) for a in l2s]
        for a in lays + l2l:
            assert L.lives_gpu_layer_pin(a) == 0
        s0 = stats(L)
        errs = []

        def track(i):
            try:
                plan_step(L, wh, H, lays[i], l2l[i], dw, dh, None, 40 + 13 * i, 2)
                assert L.lives_gpu_convert_layer_palette_full(lays[i], outpl, clamping, 0, 1, 2) == 1      # the target gamma is the layer's: no change on the way
            except Exception as e:      # noqa: BLE001
                errs.append(e)
        ths = [threading.Thread(target=track, args=(i,)) for i in range(n)]
        [t.start() for t in ths]
        [t.join() for t in ths]
        assert not errs, errs
        assert L.lives_gpu_layers_flush((ctypes.c_void_p * n)(*lays), n) == 0
        d = delta(s0, stats(L))
        if mode:
            assert d[8] == n, "every sink conversion was recorded: %s" % d
            assert (d[1], d[2], d[3], d[9], d[10], d[11]) == (1, n, 0, 1, n, 1), "one launch of lgpu_chain_to_yuv with 16 tracks: %s" % d
        else:
            assert d == [0] * 12
        out = []
        for i in range(n):
            assert L.lives_gpu_layer_sync(lays[i]) == 0
            out.append(state(wh, lays[i]))
        assert delta(s0, stats(L)) == d, "the syncs ran nothing more"
        results.append(out)
        for a in lays + l2l:
            assert L.lives_gpu_layer_unpin(a) == 0
    L.lives_gpu_set_deferred(1)
    lut = srgb_to(orc, 2)
    for i in range(n):
        equal_states(results[0][i], results[1][i], "track %d deferred / eager" % i)
        rgba = oracle_step(orc, srcs[i], sw, sh, l2s[i], dw, dh, None, 40 + 13 * i, lut, True)
        same_planes(results[0][i][1], oracle_sink(orc, rgba, dw, dh, 0, outpl, clamping), "track %d deferred / oracle" % i)


@pytest.mark.parametrize("staged", [False, True], ids=["grouped", "staged"])
@pytest.mark.parametrize("shape", [(262, 150, 128, 72, "not 2:1"), (256, 144, 128, 72, "2:1"), (256, 148, 128, 74, "2:1, dw % 8 == 0, odd chroma height"),
                                   (128, 72, 128, 72, "no resize")], ids=lambda s: s[-1])
@pytest.mark.parametrize("outpl", [YVU420P, UYVY], ids=["yvu420p", "uyvy"])
def test_every_shape_group_to_the_sink(seam, orc, deferred, tune, shape, staged, outpl):
    """groups of 3 tracks: the exact 2:1 shape in one launch; every other shape as the chain group + ONE batched conversion; SEAM_STAGED walks stages and conversions
    per track; the same bytes every way"""
    L, wh, H = seam
    sw, sh, dw, dh, _ = shape
    n = 3
    rng = np.random.default_rng(0x51D2 + sw + dh + outpl)
    srcs = [frame(rng, sw, sh, 4, alpha_mix=True) for _ in range(n)]
    l2s = [frame(rng, dw, dh, 4, alpha_mix=True) for _ in range(n)]
    if staged:
        tune("SEAM_STAGED", 1)
    lays = [wh.new_layer(BGRA32, sw, sh, [s], gamma=1) for s in srcs]
    l2l = [wh.new_layer(RGBA32, dw, dh, [a], gamma=1) for a in l2s]
    for a in lays + l2l:
        assert L.lives_gpu_layer_pin(a) == 0
    for i in range(n):
        plan_step(L, wh, H, lays[i], l2l[i], dw, dh, None, 70 + i, 2)
        assert L.lives_gpu_convert_layer_palette_full(lays[i], outpl, CLAMPED, 0, 1, 2) == 1
    s0 = stats(L)
    assert L.lives_gpu_layers_flush((ctypes.c_void_p * n)(*lays), n) == 0
    d = delta(s0, stats(L))
    if staged:
        assert (d[1], d[3], d[9], d[10], d[11]) == (0, n, n, n, 0), d
    elif (sw, sh) == (2 * dw, 2 * dh):
        assert (d[1], d[2], d[3], d[9], d[10], d[11]) == (1, n, 0, 1, n, 1), "ONE launch, and it is lgpu_chain_to_yuv: %s" % d
    else:
        assert (d[1], d[2], d[3], d[9], d[10], d[11]) == (1, n, 0, 1, n, 0), "the chain group, then one batched conversion of its RGBA frames: %s" % d
    lut = srgb_to(orc, 2)
    for i in range(n):
        assert L.lives_gpu_layer_sync(lays[i]) == 0
        rgba = oracle_step(orc, srcs[i], sw, sh, l2s[i], dw, dh, None, 70 + i, lut, True)
        same_planes(state(wh, lays[i])[1], oracle_sink(orc, rgba, dw, dh, 0, outpl, CLAMPED), "track %d" % i)
    for a in lays + l2l:
        assert L.lives_gpu_layer_unpin(a) == 0


@pytest.mark.parametrize("outpl", [YUV420P, YVU420P, UYVY], ids=["yuv420p", "yvu420p", "uyvy"])
@pytest.mark.parametrize("n,launches", [(64, 1), (65, 2), (70, 2), (130, 3)])
def test_more_tracks_than_a_launch_takes(seam, orc, deferred, outpl, n, launches):
    """one tick of 64 .. 130 pinned tracks ending at the sink, one flush.  A program that ends in LZ_SINK is registered under up to three host planes and the flush is
    handed all of them: every program must run exactly once, in lgpu_chain_to_yuv launches of at most LGPU_CHAIN_MAX_TRACKS tracks, and every track equals the oracle"""
    L, wh, H = seam
    rng = np.random.default_rng(0x51D6 + n + outpl)
    sw, sh, dw, dh = 64, 40, 32, 20
    srcs = [frame(rng, sw, sh, 4, alpha_mix=True) for _ in range(n)]
    l2s = [frame(rng, dw, dh, 4, alpha_mix=True) for _ in range(n)]
    amounts = [(17 * i + 5) % 256 for i in range(n)]
    lays = [wh.new_layer(BGRA32, sw, sh, [s], gamma=1) for s in srcs]
    l2l = [wh.new_layer(RGBA32, dw, dh, [a], gamma=1) for a in l2s]
    for a in lays + l2l:
        assert L.lives_gpu_layer_pin(a) == 0
    s0 = stats(L)
    for i in range(n):
        plan_step(L, wh, H, lays[i], l2l[i], dw, dh, None, amounts[i], 2)
        assert L.lives_gpu_convert_layer_palette_full(lays[i], outpl, CLAMPED, 0, 1, 2) == 1
    assert L.lives_gpu_layers_flush((ctypes.c_void_p * n)(*lays), n) == 0
    d = delta(s0, stats(L))
    assert d[8] == n
    assert (d[1], d[2], d[3], d[9], d[10], d[11]) == (launches, n, 0, launches, n, launches), "%d launches of lgpu_chain_to_yuv for %d tracks: %s" % (launches, n, d)
    # a second flush of the same layers, and one that lists a layer twice, find nothing to run
    assert L.lives_gpu_layers_flush((ctypes.c_void_p * (n + 1))(*(lays + [lays[0]])), n + 1) == 0
    assert delta(s0, stats(L)) == d
    lut = srgb_to(orc, 2)
    for i in range(n):
        assert L.lives_gpu_layer_sync(lays[i]) == 0
        rgba = oracle_step(orc, srcs[i], sw, sh, l2s[i], dw, dh, None, amounts[i], lut, True)
        same_planes(state(wh, lays[i])[1], oracle_sink(orc, rgba, dw, dh, 0, outpl, CLAMPED), "track %d of %d" % (i, n))
    assert delta(s0, stats(L)) == d, "the syncs ran nothing more"
    for a in lays + l2l:
        assert L.lives_gpu_layer_unpin(a) == 0


def test_sink_only_programs_share_one_batch(seam, orc, deferred):
    """16 pinned layers with no pending program, each converted to YUV420P, one flush: ONE lgpu_rgb_to_yuv_batch"""
    L, wh, H = seam
    rng = np.random.default_rng(0x51D3)
    w, h, n = 128, 72, 16
    srcs = [frame(rng, w, h, 4, alpha_mix=True) for _ in range(n)]
    lays = [wh.new_layer(RGBA32, w, h, [s], gamma=1) for s in srcs]
    for a in lays:
        assert L.lives_gpu_layer_pin(a) == 0
    s0 = stats(L)
    for a in lays:
        assert L.lives_gpu_convert_layer_palette(a, YUV420P, CLAMPED) == 1
    assert L.lives_gpu_layers_flush((ctypes.c_void_p * n)(*lays), n) == 0
    d = delta(s0, stats(L))
    assert (d[8], d[9], d[10], d[11], d[1], d[3]) == (n, 1, n, 0, 0, 0), d
    for i in range(n):
        assert L.lives_gpu_layer_sync(lays[i]) == 0
        same_planes(state(wh, lays[i])[1], oracle_sink(orc, srcs[i], w, h, 0, YUV420P, CLAMPED), "layer %d" % i)
        assert L.lives_gpu_layer_unpin(lays[i]) == 0
    assert delta(s0, stats(L)) == d


def test_a_sync_of_the_u_plane_alone_runs_the_program(seam, orc, deferred):
    """after LZ_SINK a program stands for three host planes: a layer that holds only the U plane is enough to run it"""
    L, wh, H = seam
    W = wh.weed()
    rng = np.random.default_rng(0x51D4)
    sw, sh, dw, dh = 256, 144, 128, 72
    src = frame(rng, sw, sh, 4, alpha_mix=True)
    lay = wh.new_layer(BGRA32, sw, sh, [src], gamma=1)
    assert L.lives_gpu_layer_pin(lay) == 0
    plan_step(L, wh, H, lay, None, dw, dh, None, 0, 2)
    assert L.lives_gpu_convert_layer_palette_full(lay, YUV420P, CLAMPED, 0, 1, 2) == 1
    _, ptrs, rs = wh.planes_of(lay)
    u_only = W.plant_new(128)
    for k, v in ((b"current_palette", A8), (b"width", dw // 2), (b"height", dh // 2), (b"host_gpu_resident", 1)):
        W.weed_set_int_value(u_only, k, v)
    W.weed_set_int_array(u_only, b"rowstrides", 1, (ctypes.c_int * 1)(rs[1]))
    W.weed_set_voidptr_array(u_only, b"pixel_data", 1, (ctypes.c_void_p * 1)(ptrs[1]))
    s0 = stats(L)
    assert L.lives_gpu_layer_sync(u_only) == 0
    d = delta(s0, stats(L))
    assert (d[1], d[2], d[9], d[10], d[11]) == (1, 1, 1, 1, 1), d
    rgba = oracle_step(orc, src, sw, sh, None, dw, dh, None, 0, srgb_to(orc, 2), True)
    want = oracle_sink(orc, rgba, dw, dh, 0, YUV420P, CLAMPED)
    got_u = np.frombuffer((ctypes.c_uint8 * (rs[1] * (dh // 2))).from_address(ptrs[1]), np.uint8).reshape(dh // 2, rs[1])
    assert (got_u[:, :dw // 2] == want[1]).all()
    assert L.lives_gpu_layer_sync(lay) == 0
    assert delta(s0, stats(L)) == d, "the program ran once"
    same_planes(state(wh, lay)[1], want)
    assert L.lives_gpu_layer_unpin(lay) == 0


@pytest.mark.parametrize("case", ["sync-before-flush", "second-conversion", "needed-gamma-change", "argb32", "forgotten"])
def test_interruptions(seam, orc, deferred, case):
    """whatever interrupts a pending sink program leaves bytes and leaves equal to eager execution"""
    L, wh, H = seam
    rng = np.random.default_rng(0x51D5)
    sw, sh, dw, dh = 256, 144, 128, 72
    inpl = ARGB32 if case == "argb32" else BGRA32
    src = frame(rng, sw, sh, 4, alpha_mix=True)
    l2a = frame(rng, dw, dh, 4, alpha_mix=True)
    out = []
    for mode in (1, 0):
        L.lives_gpu_set_deferred(mode)
        lay = wh.new_layer(inpl, sw, sh, [src], gamma=1)
        l2 = wh.new_layer(RGBA32, dw, dh, [l2a], gamma=1)
        assert L.lives_gpu_layer_pin(lay) == 0 and L.lives_gpu_layer_pin(l2) == 0
        s0 = stats(L)
        if case == "argb32":
            # a FALSE path: declined at record time, the layer untouched, synchronised and unpinned for the caller's CPU body
            assert L.lives_gpu_convert_layer_palette(lay, YUV420P, CLAMPED) == 0
            assert delta(s0, stats(L)) == [0] * 12
            out.append(state(wh, lay))
            assert (out[-1][1][0] == src).all() and out[-1][0][0] == ARGB32
            L.lives_gpu_layer_forget(lay)
            assert L.lives_gpu_layer_unpin(l2) == 0
            continue
        plan_step(L, wh, H, lay, l2, dw, dh, None, 99, 2)
        if case == "needed-gamma-change":
            # convert_layer_palette names no target: the layer (LINEAR after the gamma substep) goes to SRGB on the way -- today's path: materialise, then eager
            assert L.lives_gpu_convert_layer_palette(lay, YUV420P, CLAMPED) == 1
            assert delta(s0, stats(L))[8] == 0, "not recorded"
        else:
            assert L.lives_gpu_convert_layer_palette_full(lay, UYVY, CLAMPED, 0, 1, 2) == 1
            assert delta(s0, stats(L))[8] == (1 if mode else 0)
        if case == "second-conversion":
            assert L.lives_gpu_convert_layer_palette(lay, RGBA32, CLAMPED) == 1       # UYVY -> RGBA32: needs the pixels, the program runs first
        if case == "forgotten":
            s1 = stats(L)
            assert L.lives_gpu_layer_forget(lay) == 0                                  # nothing runs, and the program's three entries are gone
            d = delta(s1, stats(L))
            assert (d[1], d[3], d[9]) == (0, 0, 0), d
            assert L.lives_gpu_layer_unpin(l2) == 0
            continue
        assert L.lives_gpu_layer_sync(lay) == 0
        out.append(state(wh, lay))
        assert L.lives_gpu_layer_unpin(lay) == 0 and L.lives_gpu_layer_unpin(l2) == 0
    L.lives_gpu_set_deferred(1)
    if case != "forgotten":
        equal_states(out[0], out[1], case)
    if case == "sync-before-flush":
        rgba = oracle_step(orc, src, sw, sh, l2a, dw, dh, None, 99, srgb_to(orc, 2), True)
        same_planes(out[0][1], oracle_sink(orc, rgba, dw, dh, 0, UYVY, CLAMPED), case)
