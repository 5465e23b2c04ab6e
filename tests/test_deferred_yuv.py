"""Deferred execution of a decoder's frame on pinned layers: convert_layer_palette(YUV420P / YVU420P -> RGBA32) is recorded as the first stage of the track's program
(include/lives_gpu_layer.h) and a flush runs the tick's programs of one shape as ONE lgpu_chain_yuv420p launch in the exact 2:1 shape, as at most two launches otherwise
(the batched conversion, then lgpu_chain_amounts).  Compared three ways, as tests/test_deferred.py does: deferred == eager (lives_gpu_set_deferred(0)) == the oracle's
composition orc_yuv420p_to_rgb -> orc_pixbuf_scale -> [orc_letterbox] -> orc_blend_chroma -> orc_gamma_apply, leaves included."""
import ctypes
import threading

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.test_deferred import LEAVES, deferred, oracle_step, plan_step, seam, srgb_to, view  # noqa: F401 (fixtures)
from tests.util import frame

needs_ref = pytest.mark.skipif(not po.have_ref(), reason="oracle/_ref (reference libweed) not built")
pytestmark = [needs_ref, pytest.mark.gpu]
P = po.P
RGBA32, BGRA32, YUV420P, YVU420P, YUV422P = 3, 4, 512, 513, 522
CLAMPED, SUBSPACE_YCBCR = 0, 1


def stats(L):
    L.lives_gpu_deferred_stats_n.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    L.lives_gpu_deferred_stats_n.restype = None
    a = (ctypes.c_ulonglong * 8)()
    L.lives_gpu_deferred_stats_n(a, 8)
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


def oracle_conv(orc, Y, U, V, w, h):
    rgba = np.zeros((h, w * 4), np.uint8)
    st = (ctypes.c_int * 3)(Y.strides[0], U.strides[0], V.strides[0])
    orc.orc_yuv420p_to_rgb(P(Y), P(U), P(V), st, U.size, V.size, P(rgba), w * 4, w, h, 4, 0, 0, 0, 2, None, 0)
    return rgba


def oracle_track(orc, Y, U, V, sw, sh, l2, dw, dh, canvas, bf, lut):
    return oracle_step(orc, oracle_conv(orc, Y, U, V, sw, sh), sw, sh, l2, dw, dh, canvas, bf, lut, False)


def test_sixteen_decoder_frames_one_launch(seam, orc, deferred):
    """16 pinned YUV420P / YVU420P layers, one host thread per track, one flush: 16 YUV stages recorded, ONE chain launch carrying 16 tracks, nothing staged, no
    conversion pre-launch; bytes and leaves equal across deferred, eager and the oracle"""
    L, wh, H = seam
    rng = np.random.default_rng(0xD1)
    sw, sh, dw, dh, n = 256, 144, 128, 72, 16
    srcs = [yuv_planes(rng, sw, sh, pad=(16, 8, 24)) for _ in range(n)]
    l2s = [frame(rng, dw, dh, 4, alpha_mix=True) for _ in range(n)]
    pals = [YUV420P if i % 2 == 0 else YVU420P for i in range(n)]
    results = []
    for mode in (1, 0):
        L.lives_gpu_set_deferred(mode)
        lays = [yuv_layer(wh, pals[i], sw, sh, *srcs[i]) for i in range(n)]
        l2l = [wh.new_layer(RGBA32, dw, dh, [a], gamma=1) for a in l2s]
        for a in lays + l2l:
            assert L.lives_gpu_layer_pin(a) == 0
        s0 = stats(L)
        errs = []

        def track(i):
            try:
                plan_step(L, wh, H, lays[i], l2l[i], dw, dh, None, 40 + 13 * i, 2)
            except Exception as e:      # noqa: BLE001
                errs.append(e)
        ths = [threading.Thread(target=track, args=(i,)) for i in range(n)]
        [t.start() for t in ths]
        [t.join() for t in ths]
        assert not errs, errs
        arr = (ctypes.c_void_p * n)(*lays)
        assert L.lives_gpu_layers_flush(arr, n) == 0
        d = delta(s0, stats(L))
        if mode:
            assert d[4] == n, "every conversion was recorded"
            assert (d[1], d[2], d[3], d[5], d[6], d[7]) == (1, n, 0, 1, n, 0), "one launch of lgpu_chain_yuv420p with 16 tracks: %s" % d
        else:
            assert d == [0] * 8
        out = []
        for i in range(n):
            assert L.lives_gpu_layer_sync(lays[i]) == 0
            out.append(([wh.geti(lays[i], k) for k in LEAVES] + [wh.planes_of(lays[i])[2]], view(wh, lays[i])[:, :dw * 4].copy()))
        results.append(out)
        for a in lays + l2l:
            assert L.lives_gpu_layer_unpin(a) == 0
    L.lives_gpu_set_deferred(1)
    lut = srgb_to(orc, 2)
    for i in range(n):
        assert results[0][i][0] == results[1][i][0], "leaves, track %d" % i
        assert (results[0][i][1] == results[1][i][1]).all(), "deferred == eager, track %d" % i
        want = oracle_track(orc, *srcs[i], sw, sh, l2s[i], dw, dh, None, 40 + 13 * i, lut)
        assert (results[0][i][1] == want).all(), "deferred == oracle, track %d" % i


@pytest.mark.parametrize("n,launches", [(20, 1), (70, 2)])
def test_more_than_sixteen_decoder_frames(seam, orc, deferred, n, launches):
    """one tick of 20 / 70 pinned YUV420P / YVU420P tracks, one flush: lgpu_chain_yuv420p launches of at most LGPU_CHAIN_MAX_TRACKS tracks -- one of 20, then 64 + 6 --
    nothing staged, no conversion pre-launch, every track equal to the oracle"""
    L, wh, H = seam
    rng = np.random.default_rng(0xD6 + n)
    sw, sh, dw, dh = 128, 72, 64, 36
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
        plan_step(L, wh, H, lays[i], l2l[i], dw, dh, None, amounts[i], 2)
    assert L.lives_gpu_layers_flush((ctypes.c_void_p * n)(*lays), n) == 0
    d = delta(s0, stats(L))
    assert d[4] == n, "every conversion was recorded"
    assert (d[1], d[2], d[3], d[5], d[6], d[7]) == (launches, n, 0, launches, n, 0), "%d launches of lgpu_chain_yuv420p for %d tracks: %s" % (launches, n, d)
    lut = srgb_to(orc, 2)
    for i in range(n):
        assert L.lives_gpu_layer_sync(lays[i]) == 0
        want = oracle_track(orc, *srcs[i], sw, sh, l2s[i], dw, dh, None, amounts[i], lut)
        assert (view(wh, lays[i])[:, :dw * 4] == want).all(), "track %d of %d" % (i, n)
    for a in lays + l2l:
        assert L.lives_gpu_layer_unpin(a) == 0


SHAPES = [
    # sw, sh, dw, dh, canvas, with layer 2, gamma target, note
    (262, 150, 128, 72, None, True, 2, "not 2:1"),
    (128, 72, 128, 72, None, True, 2, "no resize"),
    (128, 72, 128, 72, (160, 100), True, None, "letterbox only"),
    (128, 72, 128, 72, None, False, None, "conversion only"),
    (256, 144, 128, 72, (132, 80), False, 2, "2:1 into a canvas, no blend: one launch"),
]


@pytest.mark.parametrize("staged", [False, True], ids=["grouped", "staged"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[-1] for s in SHAPES])
def test_every_shape_group(seam, orc, deferred, tune, shape, staged):
    """each shape's group of 3 tracks: correct bytes; the exact 2:1 shape in one launch, every other in at most two (the conversion batch + the chain); with
    SEAM_STAGED the YUV stage is walked one call at a time as well"""
    L, wh, H = seam
    sw, sh, dw, dh, canvas, with_l2, gamma, _ = shape
    n = 3
    rng = np.random.default_rng(0xD2 + sw + dh + (canvas[0] if canvas else 0))
    ow, oh = canvas if canvas else (dw, dh)
    srcs = [yuv_planes(rng, sw, sh, pad=(4, 2, 6)) for _ in range(n)]
    l2s = [frame(rng, ow, oh, 4, alpha_mix=True) for _ in range(n)]
    if staged:
        tune("SEAM_STAGED", 1)
    lays = [yuv_layer(wh, YUV420P, sw, sh, *s) for s in srcs]
    l2l = [wh.new_layer(RGBA32, ow, oh, [a], gamma=1) for a in l2s] if with_l2 else [None] * n
    for a in lays + [x for x in l2l if x is not None]:
        assert L.lives_gpu_layer_pin(a) == 0
    for i in range(n):
        plan_step(L, wh, H, lays[i], l2l[i], dw, dh, canvas, 70 + i, gamma)
    s0 = stats(L)
    assert L.lives_gpu_layers_flush((ctypes.c_void_p * n)(*lays), n) == 0
    d = delta(s0, stats(L))
    fused = (sw, sh) == (2 * dw, 2 * dh)
    if staged:
        assert (d[1], d[5], d[7]) == (0, 0, 0) and d[3] == (0 if shape[-1] == "conversion only" else n), d
    elif fused:
        assert (d[1], d[2], d[5], d[6], d[7], d[3]) == (1, n, 1, n, 0, 0), d
    else:
        assert d[7] == 1 and d[5] == 0 and d[3] == 0 and d[1] <= 1 and d[7] + d[1] <= 2, "at most two launches for the group: %s" % d
    lut = srgb_to(orc, gamma) if gamma is not None else None
    for i in range(n):
        assert L.lives_gpu_layer_sync(lays[i]) == 0
        want = oracle_track(orc, *srcs[i], sw, sh, l2s[i] if with_l2 else None, dw, dh, canvas, 70 + i, lut)
        assert (view(wh, lays[i])[:, :ow * 4] == want).all(), i
    for a in lays + [x for x in l2l if x is not None]:
        assert L.lives_gpu_layer_unpin(a) == 0


def test_interruptions(seam, orc, deferred):
    """a pending conversion runs when its pixels are needed (sync, alpha_premult), and runs nothing when the layer is forgotten"""
    L, wh, H = seam
    rng = np.random.default_rng(0xD3)
    sw, sh = 256, 144
    Y, U, V = yuv_planes(rng, sw, sh)
    want = oracle_conv(orc, Y, U, V, sw, sh)
    # sync straight after the convert
    lay = yuv_layer(wh, YUV420P, sw, sh, Y, U, V)
    assert L.lives_gpu_layer_pin(lay) == 0
    s0 = stats(L)
    assert L.lives_gpu_convert_layer_palette(lay, RGBA32, 0) == 1
    assert delta(s0, stats(L))[4] == 1
    assert L.lives_gpu_layer_sync(lay) == 0
    assert (view(wh, lay)[:, :sw * 4] == want).all()
    assert L.lives_gpu_layer_unpin(lay) == 0
    # alpha_premult after the convert: the program runs first, the premultiply sees its result
    outs = []
    for mode in (1, 0):
        L.lives_gpu_set_deferred(mode)
        lay = yuv_layer(wh, YUV420P, sw, sh, Y, U, V)
        assert L.lives_gpu_layer_pin(lay) == 0
        assert L.lives_gpu_convert_layer_palette(lay, RGBA32, 0) == 1
        L.lives_gpu_alpha_premult(lay, 1)
        assert L.lives_gpu_layer_sync(lay) == 0
        outs.append(([wh.geti(lay, k) for k in LEAVES], view(wh, lay)[:, :sw * 4].copy()))
        assert L.lives_gpu_layer_unpin(lay) == 0
    L.lives_gpu_set_deferred(1)
    assert outs[0][0] == outs[1][0] and (outs[0][1] == outs[1][1]).all()
    b = want.copy()
    orc.orc_alpha_premult(P(b), sw * 4, sw, sh, 0, 0)
    assert (outs[0][1] == b).all()
    # forgotten while pending: nothing runs
    lay = yuv_layer(wh, YVU420P, sw, sh, Y, U, V)
    assert L.lives_gpu_layer_pin(lay) == 0
    assert L.lives_gpu_convert_layer_palette(lay, BGRA32, 0) == 1 and L.lives_gpu_resize_layer(lay, 128, 72, 3, BGRA32, 0) == 1
    s0 = stats(L)
    assert L.lives_gpu_layer_forget(lay) == 0
    d = delta(s0, stats(L))
    assert (d[1], d[3], d[5], d[7]) == (0, 0, 0, 0), d


def test_decoder_surfaces_in_hbm(seam, orc, deferred, gpu):
    """lives_gpu_layer_pin_device with the three planes of a decoder surface: no upload, one launch, the surfaces are read and never written, and serve the next tick"""
    import torch
    from tests.util import dev, host
    L, wh, H = seam
    rng = np.random.default_rng(0xD4)
    sw, sh, dw, dh = 256, 144, 128, 72
    Y, U, V = yuv_planes(rng, sw, sh, pad=(0, 0, 0))
    l2a = frame(rng, dw, dh, 4, alpha_mix=True)
    dY, dU, dV = dev(Y), dev(U), dev(V)
    torch.cuda.synchronize()
    want = oracle_track(orc, Y, U, V, sw, sh, l2a, dw, dh, None, 128, srgb_to(orc, 2))
    h2d0 = ctypes.c_ulonglong()
    for tick in range(3):
        lay = yuv_layer(wh, YUV420P, sw, sh, np.zeros_like(Y), np.zeros_like(U), np.zeros_like(V))
        l2 = wh.new_layer(RGBA32, dw, dh, [l2a], gamma=1)
        assert L.lives_gpu_layer_pin(l2) == 0
        if tick == 0:
            L.lives_gpu_transfer_stats(ctypes.byref(h2d0), None)
        pl = (ctypes.c_void_p * 3)(dY.data_ptr(), dU.data_ptr(), dV.data_ptr())
        assert L.lives_gpu_layer_pin_device(lay, pl, 3, None, 1) == 0
        s0 = stats(L)
        plan_step(L, wh, H, lay, l2, dw, dh, None, 128, 2)
        assert L.lives_gpu_layers_flush((ctypes.c_void_p * 1)(lay), 1) == 0
        d = delta(s0, stats(L))
        assert (d[4], d[5], d[6], d[7]) == (1, 1, 1, 0), d
        assert L.lives_gpu_layer_sync(lay) == 0
        assert (view(wh, lay)[:, :dw * 4] == want).all(), tick
        assert L.lives_gpu_layer_forget(lay) == 0 and L.lives_gpu_layer_forget(l2) == 0
        if tick == 0:
            h2d1 = ctypes.c_ulonglong()
            L.lives_gpu_transfer_stats(ctypes.byref(h2d1), None)
            assert h2d1.value == h2d0.value, "the surfaces were not uploaded"
    assert (host(dY) == Y).all() and (host(dU) == U).all() and (host(dV) == V).all(), "the caller's surfaces are as they were"


@pytest.mark.parametrize("case", ["target-gamma", "yuv422p"])
def test_still_eager(seam, orc, deferred, case):
    """a conversion with a target gamma (the fused 16-bit LUT) and a YUV422P frame are not recorded: they run as before, with the same bytes in both modes"""
    L, wh, H = seam
    rng = np.random.default_rng(0xD5)
    sw, sh = 128, 72
    pal = YUV422P if case == "yuv422p" else YUV420P
    Y = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
    ch = sh if pal == YUV422P else sh // 2
    U = rng.integers(0, 256, (ch, sw // 2), dtype=np.uint8)
    V = rng.integers(0, 256, (ch, sw // 2), dtype=np.uint8)
    outs = []
    for mode in (1, 0):
        L.lives_gpu_set_deferred(mode)
        lay = wh.new_layer(pal, sw, sh, [Y, U, V], gamma=1, clamping=CLAMPED, subspace=SUBSPACE_YCBCR)
        assert L.lives_gpu_layer_pin(lay) == 0
        s0 = stats(L)
        if case == "target-gamma":
            assert L.lives_gpu_convert_layer_palette_full(lay, RGBA32, 0, 0, 0, 2) == 1
        else:
            assert L.lives_gpu_convert_layer_palette(lay, RGBA32, 0) == 1
        assert delta(s0, stats(L)) == [0] * 8, "nothing recorded"
        assert L.lives_gpu_layer_sync(lay) == 0
        outs.append(([wh.geti(lay, k) for k in LEAVES], view(wh, lay)[:, :sw * 4].copy()))
        assert L.lives_gpu_layer_unpin(lay) == 0
    L.lives_gpu_set_deferred(1)
    assert outs[0][0] == outs[1][0] and (outs[0][1] == outs[1][1]).all()
    if case == "yuv422p":
        want = np.zeros((sh, sw * 4), np.uint8)
        st = (ctypes.c_int * 3)(sw, sw // 2, sw // 2)
        orc.orc_yuv420p_to_rgb(P(Y), P(U), P(V), st, U.size, V.size, P(want), sw * 4, sw, sh, 4, 0, 1, 0, 2, None, 0)
        assert (outs[0][1] == want).all()
