"""Deferred execution of a whole tick on pinned layers, from a decoder's frame to the consumer's palette: convert_layer_palette(YUV420P / YVU420P -> RGBA32 / BGRA32)
-> resize 2:1 -> the "chroma blend" process_func -> gamma_convert_layer -> convert_layer_palette_full(-> YUV420P / YVU420P / UYVY / YUYV) is recorded as one program
per track (LZ_YUV .. LZ_SINK, include/lives_gpu_layer.h) and a flush runs the tick's programs of one shape as ONE lgpu_chain_yuv420p_to_yuv launch -- from YUV planes
to YUV planes, no RGBA frame at either end -- for the sink formats the seam has chosen it for (FUSED below), as lgpu_chain_yuv420p + one batched conversion for the
others.  Compared three ways, as tests/test_deferred.py does: deferred == eager (lives_gpu_set_deferred(0)) == the oracle's
composition orc_yuv420p_to_rgb -> orc_pixbuf_scale -> orc_blend_chroma -> orc_gamma_apply -> orc_rgb_to_yuv, on every plane and on the layer's leaves."""
import ctypes
import threading

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.test_deferred import OURS, deferred, oracle_step, plan_step, seam, srgb_to, view  # noqa: F401 (fixtures)
from tests.util import frame

pytestmark = pytest.mark.gpu
P = po.P
RGBA32, BGRA32, YUV420P, YVU420P, UYVY, YUYV = 3, 4, 512, 513, 564, 565
K4_FMT = {YUV420P: 4, YVU420P: 4, UYVY: 2, YUYV: 3}
CLAMPED, UNCLAMPED, SUBSPACE_YCBCR = 0, 1, 1
SINK_LEAVES = ("current_palette", "width", "height", "YUV_clamping", "YUV_subspace", "YUV_sampling", "gamma_type", "host_flags")
SINKS = [YUV420P, YVU420P, UYVY, YUYV]
# the seam's choice per sink format: True -- a group in the one-launch form runs as lgpu_chain_yuv420p_to_yuv.  profiles/r09/transcode_chain.md (16 x 4K -> 1080p, blend
# + LUT): to UYVY the one launch takes 214.3 us against 244.7 for lgpu_chain_yuv420p + lgpu_rgb_to_yuv_batch (spread 0.2 us) and the seam takes it, for YUYV too (the same
# kernel instantiation); to YUV420P it takes 258.9 us against 243.4 (spread 1.9 us), so the seam keeps the two launches for the planar sinks (seam_lazy.cpp,
# lazy_run_sink) and the counters below expect that; the planar launch itself is held against the oracle in tests/test_chain_transcode.py
FUSED = {YUV420P: False, YVU420P: False, UYVY: True, YUYV: True}
PER_LAUNCH = 32            # LGPU_CHAIN_TRANSCODE_TRACKS: tracks per launch of lgpu_chain_yuv420p_to_yuv (the counters count launches)


def stats(L):
    L.lives_gpu_deferred_stats_n.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    L.lives_gpu_deferred_stats_n.restype = None
    a = (ctypes.c_ulonglong * 13)()
    L.lives_gpu_deferred_stats_n(a, 13)
    return list(a)


def delta(a, b):
    return [y - x for x, y in zip(a, b)]


def yuv_planes(rng, w, h, pad=(0, 0, 0)):
    Y = rng.integers(0, 256, (h, w + pad[0]), dtype=np.uint8)
    U = rng.integers(0, 256, (h // 2, w // 2 + pad[1]), dtype=np.uint8)
    V = rng.integers(0, 256, (h // 2, w // 2 + pad[2]), dtype=np.uint8)
    return Y, U, V


def yuv_layer(wh, pal, w, h, Y, U, V):
    """the layer's planes in its palette's order: YVU420P stores V second"""
    return wh.new_layer(pal, w, h, [Y, V, U] if pal == YVU420P else [Y, U, V], gamma=1, clamping=CLAMPED, subspace=SUBSPACE_YCBCR)


def oracle_track(orc, Y, U, V, sw, sh, mid, l2, dw, dh, canvas, bf, lut, outpl, clamping):
    """one track: K2 into the middle palette's byte order, the RGBA stages, K4 into compact planes in the LAYER's plane order (YVU420P stores V second)"""
    order = 1 if mid == BGRA32 else 0
    rgba = np.zeros((sh, sw * 4), np.uint8)
    st = (ctypes.c_int * 3)(Y.strides[0], U.strides[0], V.strides[0])
    orc.orc_yuv420p_to_rgb(P(Y), P(U), P(V), st, U.size, V.size, P(rgba), sw * 4, sw, sh, 4, order, 0, 0, 2, None, 0)
    out = oracle_step(orc, rgba, sw, sh, l2, dw, dh, canvas, bf, lut, False)
    w, h = canvas if canvas else (dw, dh)
    fmt = K4_FMT[outpl]
    if fmt == 4:
        w, h = w & ~1, h & ~1
    want, _ = po.k4_out_planes(0, w, h, fmt, 0)
    wp, ws = po.planes_args(want)
    assert orc.orc_rgb_to_yuv(P(out), out.strides[0], w, h, order, 1, ctypes.addressof(wp), ctypes.addressof(ws), fmt, 0, 1 if clamping == UNCLAMPED else 0) == 0
    return [want[0], want[2], want[1]] if outpl == YVU420P else want


def tick_calls(L, wh, H, lay, l2, mid, dw, dh, canvas, bf, outpl, clamping, between=None):
    """the calls of one track: the plan step (conversion to `mid`, resize, [letterbox], chroma blend, gamma) and the hand-over to the sink's palette; the target gamma
    is the layer's, so there is no change on the way"""
    plan_step(L, wh, H, lay, l2, dw, dh, canvas, bf, 2, swap_to=mid)
    if between:
        between()
    assert L.lives_gpu_convert_layer_palette_full(lay, outpl, clamping, 0, 1, 2) == 1


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
@pytest.mark.parametrize("mid", [RGBA32, BGRA32], ids=["rgba", "bgra"])
def test_sixteen_track_tick_from_yuv_to_yuv(seam, orc, deferred, outpl, mid):
    """16 pinned YUV420P / YVU420P tracks, one host thread per track, one flush: 16 YUV stages and 16 sink stages recorded; to the packed sinks ONE launch carrying 16
    tracks which is the chain launch [1], the YUV launch [5], the sink launch [9], fused [11] and from YUV to YUV [12]; to the planar sinks (FUSED above) one
    lgpu_chain_yuv420p launch and one batched conversion; nothing staged [3], no conversion pre-launch [7]; the later syncs run nothing more; planes and leaves equal
    across deferred, eager and the oracle"""
    L, wh, H = seam
    rng = np.random.default_rng(0x7C0 + outpl + mid)
    sw, sh, dw, dh, n = 256, 144, 128, 72, 16
    srcs = [yuv_planes(rng, sw, sh, pad=(16, 8, 24)) for _ in range(n)]
    l2s = [frame(rng, dw, dh, 4, alpha_mix=True) for _ in range(n)]
    pals = [YUV420P if i % 2 == 0 else YVU420P for i in range(n)]
    clamping = UNCLAMPED if outpl in (YVU420P, YUYV) else CLAMPED
    results = []
    for mode in (1, 0):
        L.lives_gpu_set_deferred(mode)
        lays = [yuv_layer(wh, pals[i], sw, sh, *srcs[i]) for i in range(n)]
        l2l = [wh.new_layer(mid, dw, dh, [a], gamma=1) for a in l2s]
        for a in lays + l2l:
            assert L.lives_gpu_layer_pin(a) == 0
        s0 = stats(L)
        errs = []

        def track(i):
            try:
                tick_calls(L, wh, H, lays[i], l2l[i], mid, dw, dh, None, 40 + 13 * i, outpl, clamping)
            except Exception as e:      # noqa: BLE001
                errs.append(e)
        ths = [threading.Thread(target=track, args=(i,)) for i in range(n)]
        [t.start() for t in ths]
        [t.join() for t in ths]
        assert not errs, errs
        assert L.lives_gpu_layers_flush((ctypes.c_void_p * n)(*lays), n) == 0
        d = delta(s0, stats(L))
        if mode:
            assert (d[4], d[8]) == (n, n), "every conversion was recorded, at both ends: %s" % d
            if FUSED[outpl]:
                assert (d[1], d[5], d[9], d[11], d[12]) == (1, 1, 1, 1, 1), "ONE launch, and it is lgpu_chain_yuv420p_to_yuv: %s" % d
                assert (d[2], d[6], d[10]) == (n, n, n), "it carries 16 tracks: %s" % d
                assert (d[3], d[7]) == (0, 0), "nothing staged, no conversion pre-launch: %s" % d
            else:
                assert (d[1], d[5], d[9], d[11], d[12], d[3], d[7]) == (1, 1, 1, 0, 0, 0, 0), "lgpu_chain_yuv420p, then one batched conversion: %s" % d
        else:
            assert d == [0] * 13
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
        want = oracle_track(orc, *srcs[i], sw, sh, mid, l2s[i], dw, dh, None, 40 + 13 * i, lut, outpl, clamping)
        same_planes(results[0][i][1], want, "track %d deferred / oracle" % i)


def test_twelve_counters_are_what_they_were(seam, deferred):
    """a caller that passes n = 12 gets twelve entries and the thirteenth slot of its array is left alone"""
    L = seam[0]
    L.lives_gpu_deferred_stats_n.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    L.lives_gpu_deferred_stats_n.restype = None
    a = (ctypes.c_ulonglong * 13)(*([0xA5A5] * 13))
    L.lives_gpu_deferred_stats_n(a, 12)
    assert a[12] == 0xA5A5 and list(a)[:12] == stats(L)[:12]


FALLBACK = [
    # sw, sh, dw, dh, canvas, note
    (262, 150, 128, 72, None, "not 2:1"),
    (128, 72, 128, 72, None, "no resize"),
    (256, 144, 128, 72, (132, 80), "2:1 into a letterbox canvas"),
]


@pytest.mark.parametrize("shape", FALLBACK, ids=[s[-1] for s in FALLBACK])
@pytest.mark.parametrize("outpl", [YVU420P, UYVY], ids=["yvu420p", "uyvy"])
def test_shapes_outside_the_form_keep_their_launches(seam, orc, deferred, shape, outpl):
    """groups of 3 tracks at shapes the one-launch form does not take: no launch from YUV to YUV, the launches of before, and the oracle's bytes"""
    L, wh, H = seam
    sw, sh, dw, dh, canvas, _ = shape
    n = 3
    rng = np.random.default_rng(0x7C2 + sw + dh + outpl + (canvas[0] if canvas else 0))
    ow, oh = canvas if canvas else (dw, dh)
    srcs = [yuv_planes(rng, sw, sh, pad=(4, 2, 6)) for _ in range(n)]
    l2s = [frame(rng, ow, oh, 4, alpha_mix=True) for _ in range(n)]
    lays = [yuv_layer(wh, YUV420P, sw, sh, *s) for s in srcs]
    l2l = [wh.new_layer(RGBA32, ow, oh, [a], gamma=1) for a in l2s]
    for a in lays + l2l:
        assert L.lives_gpu_layer_pin(a) == 0
    for i in range(n):
        tick_calls(L, wh, H, lays[i], l2l[i], RGBA32, dw, dh, canvas, 70 + i, outpl, CLAMPED)
    s0 = stats(L)
    assert L.lives_gpu_layers_flush((ctypes.c_void_p * n)(*lays), n) == 0
    d = delta(s0, stats(L))
    assert d[12] == 0 and d[11] == 0, "no fused sink launch: %s" % d
    assert (d[3], d[9], d[10]) == (0, 1, n), "nothing staged, one batched conversion to the sink: %s" % d
    if canvas:
        assert (d[1], d[5], d[7]) == (1, 1, 0), "lgpu_chain_yuv420p into the canvas: %s" % d
    else:
        assert (d[5], d[7]) == (0, 1) and d[1] <= 1, "the conversion batch, then the chain: %s" % d
    lut = srgb_to(orc, 2)
    for i in range(n):
        assert L.lives_gpu_layer_sync(lays[i]) == 0
        want = oracle_track(orc, *srcs[i], sw, sh, RGBA32, l2s[i], dw, dh, canvas, 70 + i, lut, outpl, CLAMPED)
        same_planes(state(wh, lays[i])[1], want, "track %d" % i)
    for a in lays + l2l:
        assert L.lives_gpu_layer_unpin(a) == 0


@pytest.mark.parametrize("outpl", SINKS, ids=["yuv420p", "yvu420p", "uyvy", "yuyv"])
def test_staged_walk_gives_the_same_bytes(seam, orc, deferred, tune, outpl):
    """SEAM_STAGED keeps walking stage by stage -- no fused launch of any kind -- and gives the oracle's bytes"""
    L, wh, H = seam
    rng = np.random.default_rng(0x7C3 + outpl)
    sw, sh, dw, dh, n = 256, 148, 128, 74, 3
    srcs = [yuv_planes(rng, sw, sh, pad=(4, 2, 6)) for _ in range(n)]
    l2s = [frame(rng, dw, dh, 4, alpha_mix=True) for _ in range(n)]
    tune("SEAM_STAGED", 1)
    lays = [yuv_layer(wh, YVU420P, sw, sh, *s) for s in srcs]
    l2l = [wh.new_layer(BGRA32, dw, dh, [a], gamma=1) for a in l2s]
    for a in lays + l2l:
        assert L.lives_gpu_layer_pin(a) == 0
    for i in range(n):
        tick_calls(L, wh, H, lays[i], l2l[i], BGRA32, dw, dh, None, 90 + i, outpl, CLAMPED)
    s0 = stats(L)
    assert L.lives_gpu_layers_flush((ctypes.c_void_p * n)(*lays), n) == 0
    d = delta(s0, stats(L))
    assert (d[1], d[5], d[7], d[11], d[12]) == (0, 0, 0, 0, 0) and (d[3], d[9], d[10]) == (n, n, n), d
    lut = srgb_to(orc, 2)
    for i in range(n):
        assert L.lives_gpu_layer_sync(lays[i]) == 0
        want = oracle_track(orc, *srcs[i], sw, sh, BGRA32, l2s[i], dw, dh, None, 90 + i, lut, outpl, CLAMPED)
        same_planes(state(wh, lays[i])[1], want, "track %d" % i)
    for a in lays + l2l:
        assert L.lives_gpu_layer_unpin(a) == 0


def test_a_host_read_between_the_stages_interrupts_the_program(seam, orc, deferred):
    """the host reads the layer's plane after the resize (a sync): the program so far runs as lgpu_chain_yuv420p, the rest is a new program that ends at the sink with an
    RGBA source -- no launch from YUV to YUV, and bytes and leaves equal to eager execution and the oracle"""
    L, wh, H = seam
    rng = np.random.default_rng(0x7C4)
    sw, sh, dw, dh = 256, 144, 128, 72
    Y, U, V = yuv_planes(rng, sw, sh, pad=(8, 4, 12))
    l2a = frame(rng, dw, dh, 4, alpha_mix=True)
    out = []
    for mode in (1, 0):
        L.lives_gpu_set_deferred(mode)
        lay = yuv_layer(wh, YUV420P, sw, sh, Y, U, V)
        l2 = wh.new_layer(RGBA32, dw, dh, [l2a], gamma=1)
        assert L.lives_gpu_layer_pin(lay) == 0 and L.lives_gpu_layer_pin(l2) == 0
        s0 = stats(L)
        assert L.lives_gpu_convert_layer_palette(lay, RGBA32, 0) == 1
        assert L.lives_gpu_resize_layer(lay, dw, dh, 3, RGBA32, 0) == 1
        assert L.lives_gpu_layer_sync(lay) == 0                   # the host looks at the scaled frame
        d = delta(s0, stats(L))
        assert (d[5], d[6], d[12]) == ((1, 1, 0) if mode else (0, 0, 0)), d
        v, v2 = view(wh, lay), view(wh, l2)
        H.run(OURS, "chroma blend", RGBA32, dw, dh, [v, v2], v, [po.p_int(99)])
        assert L.lives_gpu_gamma_convert_layer(2, lay) == 1
        assert L.lives_gpu_convert_layer_palette_full(lay, UYVY, CLAMPED, 0, 1, 2) == 1
        assert L.lives_gpu_layer_sync(lay) == 0
        d = delta(s0, stats(L))
        assert d[12] == 0, d
        out.append(state(wh, lay))
        assert L.lives_gpu_layer_unpin(lay) == 0 and L.lives_gpu_layer_unpin(l2) == 0
    L.lives_gpu_set_deferred(1)
    equal_states(out[0], out[1], "deferred / eager")
    same_planes(out[0][1], oracle_track(orc, Y, U, V, sw, sh, RGBA32, l2a, dw, dh, None, 99, srgb_to(orc, 2), UYVY, CLAMPED), "deferred / oracle")


@pytest.mark.parametrize("outpl", [YUV420P, UYVY], ids=["yuv420p", "uyvy"])
def test_a_tick_of_65_tracks_splits(seam, orc, deferred, outpl):
    """65 pinned tracks from YUV to YUV, one flush: every program runs exactly once, in groups of at most LGPU_CHAIN_MAX_TRACKS tracks (64 + 1) -- the one-launch form
    in launches of at most 32 (32 + 32, then 1) -- and every track equals the oracle"""
    L, wh, H = seam
    n = 65
    rng = np.random.default_rng(0x7C5 + outpl)
    sw, sh, dw, dh = 64, 40, 32, 20
    srcs = [yuv_planes(rng, sw, sh, pad=(8, 4, 12)) for _ in range(n)]
    l2s = [frame(rng, dw, dh, 4, alpha_mix=True) for _ in range(n)]
    pals = [YUV420P if i % 3 else YVU420P for i in range(n)]
    amounts = [(17 * i + 5) % 256 for i in range(n)]
    lays = [yuv_layer(wh, pals[i], sw, sh, *srcs[i]) for i in range(n)]
    l2l = [wh.new_layer(RGBA32, dw, dh, [a], gamma=1) for a in l2s]
    for a in lays + l2l:
        assert L.lives_gpu_layer_pin(a) == 0
    s0 = stats(L)
    for i in range(n):
        tick_calls(L, wh, H, lays[i], l2l[i], RGBA32, dw, dh, None, amounts[i], outpl, CLAMPED)
    assert L.lives_gpu_layers_flush((ctypes.c_void_p * n)(*lays), n) == 0
    d = delta(s0, stats(L))
    assert (d[4], d[8]) == (n, n)
    if FUSED[outpl]:
        nl = -(-64 // PER_LAUNCH) + 1
        assert (d[1], d[5], d[9], d[11], d[12]) == (nl,) * 5 and (d[2], d[6], d[10]) == (n, n, n) and (d[3], d[7]) == (0, 0), d
    else:
        assert (d[1], d[5], d[12], d[3], d[7]) == (2, 2, 0, 0, 0) and (d[2], d[6], d[10]) == (n, n, n), d
    lut = srgb_to(orc, 2)
    for i in range(n):
        assert L.lives_gpu_layer_sync(lays[i]) == 0
        want = oracle_track(orc, *srcs[i], sw, sh, RGBA32, l2s[i], dw, dh, None, amounts[i], lut, outpl, CLAMPED)
        same_planes(state(wh, lays[i])[1], want, "track %d of %d" % (i, n))
    assert delta(s0, stats(L)) == d, "the syncs ran nothing more"
    for a in lays + l2l:
        assert L.lives_gpu_layer_unpin(a) == 0
