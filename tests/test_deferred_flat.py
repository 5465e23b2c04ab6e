"""lives_gpu_set_flat_yuv(1): a flush runs a group of decoder frames that KEEP their size (YUV420P / YVU420P -> RGBA32 / BGRA32, letterboxed or not, blend, gamma) as
ONE lgpu_chain_flat_yuv420p launch, and such a group that ends in a YUV sink as ONE lgpu_chain_flat_yuv420p_to_yuv launch -- no conversion pre-launch, no RGBA frame.
Off (the default) the launches and counters are today's; SEAM_STAGED still wins.  Compared three ways, as tests/test_deferred.py does: deferred == eager
(lives_gpu_set_deferred(0)) == the oracle's composition, leaves included."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.test_deferred import LEAVES, deferred, plan_step, seam, srgb_to, view  # noqa: F401 (fixtures)
from tests.test_deferred_transcode import equal_states, same_planes, state, tick_calls
from tests.test_deferred_transcode import oracle_track as oracle_sink_track
from tests.test_deferred_yuv import oracle_track, yuv_layer, yuv_planes
from tests.util import frame

needs_ref = pytest.mark.skipif(not po.have_ref(), reason="oracle/_ref (reference libweed) not built")
pytestmark = [needs_ref, pytest.mark.gpu]
RGBA32, BGRA32, YUV420P, YVU420P, UYVY, YUYV = 3, 4, 512, 513, 564, 565
CLAMPED, UNCLAMPED = 0, 1
NSTATS = 15
# the sink formats lives_gpu_set_flat_yuv(1) routes to the one launch (seam_lazy.cpp, FLAT_SINK_FORMATS: those tools/bench_flat_chain.py shows ahead of today's
# three launches, profiles/r11/flat_chain.md: 157.2 us against 274.2 to UYVY, 159.7 against 271.7 to YUV420P, spreads below 1 us -- all taken); YUV420P: 32 tracks per launch
FLAT_SINK = {UYVY: True, YUYV: True, YUV420P: True, YVU420P: True}


def stats(L):
    L.lives_gpu_deferred_stats_n.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    L.lives_gpu_deferred_stats_n.restype = None
    a = (ctypes.c_ulonglong * NSTATS)()
    L.lives_gpu_deferred_stats_n(a, NSTATS)
    return list(a)


def delta(a, b):
    return [y - x for x, y in zip(a, b)]


@pytest.fixture()
def flat(seam):
    """set / restore lives_gpu_set_flat_yuv around a test; off is the default"""
    L = seam[0]
    L.lives_gpu_set_flat_yuv.argtypes = [ctypes.c_int]
    L.lives_gpu_set_flat_yuv.restype = ctypes.c_int
    prev = L.lives_gpu_set_flat_yuv(0)
    try:
        assert prev == 0, "the flat route is off by default"
        yield L.lives_gpu_set_flat_yuv
    finally:
        L.lives_gpu_set_flat_yuv(0)


RGBA_SHAPES = [
    # w, h, canvas, gamma target, note (tests/test_deferred_yuv.py SHAPES)
    (128, 72, None, 2, "no resize"),
    (128, 72, (160, 100), None, "letterbox only"),
]


def rgba_group(L, wh, H, orc, shape, n, seed):
    """n tracks of one unscaled shape, deferred and eager: (counter deltas of the deferred flush, results[mode][track] = (leaves, bytes), oracle bytes per track)"""
    w, h, canvas, gamma, _ = shape
    rng = np.random.default_rng(seed)
    ow, oh = canvas if canvas else (w, h)
    srcs = [yuv_planes(rng, w, h, pad=(4, 2, 6)) for _ in range(n)]
    l2s = [frame(rng, ow, oh, 4, alpha_mix=True) for _ in range(n)]
    pals = [YUV420P if i % 2 == 0 else YVU420P for i in range(n)]
    results, d = [], None
    try:
        for mode in (1, 0):
            L.lives_gpu_set_deferred(mode)
            lays = [yuv_layer(wh, pals[i], w, h, *srcs[i]) for i in range(n)]
            l2l = [wh.new_layer(RGBA32, ow, oh, [a], gamma=1) for a in l2s]
            for a in lays + l2l:
                assert L.lives_gpu_layer_pin(a) == 0
            s0 = stats(L)
            for i in range(n):
                plan_step(L, wh, H, lays[i], l2l[i], w, h, canvas, 40 + 13 * i, gamma)
            assert L.lives_gpu_layers_flush((ctypes.c_void_p * n)(*lays), n) == 0
            if mode:
                d = delta(s0, stats(L))
            else:
                assert delta(s0, stats(L)) == [0] * NSTATS
            out = []
            for i in range(n):
                assert L.lives_gpu_layer_sync(lays[i]) == 0
                out.append(([wh.geti(lays[i], k) for k in LEAVES] + [wh.planes_of(lays[i])[2]], view(wh, lays[i])[:, :ow * 4].copy()))
            results.append(out)
            for a in lays + l2l:
                assert L.lives_gpu_layer_unpin(a) == 0
    finally:
        L.lives_gpu_set_deferred(1)
    lut = srgb_to(orc, gamma) if gamma is not None else None
    wants = [oracle_track(orc, *srcs[i], w, h, l2s[i], w, h, canvas, 40 + 13 * i, lut) for i in range(n)]
    return d, results, wants


def check_rgba(results, wants):
    for i, want in enumerate(wants):
        assert results[0][i][0] == results[1][i][0], "leaves, track %d" % i
        assert (results[0][i][1] == results[1][i][1]).all(), "deferred == eager, track %d" % i
        assert (results[0][i][1] == want).all(), "deferred == oracle, track %d" % i


@pytest.mark.parametrize("n", [3, 16])
@pytest.mark.parametrize("shape", RGBA_SHAPES, ids=[s[-1] for s in RGBA_SHAPES])
def test_flat_rgba_group_is_one_launch(seam, orc, deferred, flat, shape, n):
    """the "no resize" and "letterbox only" shapes with the route on: ONE chain launch [1] carrying n tracks [2], which is the flat launch [13] / [14]; no conversion
    pre-launch [7], no 2:1 YUV launch [5], nothing staged [3]; bytes and leaves equal across deferred, eager and the oracle"""
    L, wh, H = seam
    assert flat(1) == 0
    d, results, wants = rgba_group(L, wh, H, orc, shape, n, 0xF1 + n + (shape[2][0] if shape[2] else 0))
    assert d[4] == n, "every conversion was recorded"
    assert (d[1], d[2], d[3], d[5], d[7], d[13], d[14]) == (1, n, 0, 0, 0, 1, n), "one lgpu_chain_flat_yuv420p launch with %d tracks: %s" % (n, d)
    check_rgba(results, wants)


SINK_CASES = [(UYVY, RGBA32, CLAMPED), (YUV420P, BGRA32, CLAMPED), (YVU420P, RGBA32, UNCLAMPED), (YUYV, BGRA32, UNCLAMPED)]


def sink_group(L, wh, H, orc, outpl, mid, clamping, n, seed):
    """n unscaled tracks ("no resize", blend, gamma) that end in the sink palette, deferred and eager"""
    w, h = 128, 72
    rng = np.random.default_rng(seed)
    srcs = [yuv_planes(rng, w, h, pad=(16, 8, 24)) for _ in range(n)]
    l2s = [frame(rng, w, h, 4, alpha_mix=True) for _ in range(n)]
    pals = [YUV420P if i % 2 == 0 else YVU420P for i in range(n)]
    results, d = [], None
    try:
        for mode in (1, 0):
            L.lives_gpu_set_deferred(mode)
            lays = [yuv_layer(wh, pals[i], w, h, *srcs[i]) for i in range(n)]
            l2l = [wh.new_layer(mid, w, h, [a], gamma=1) for a in l2s]
            for a in lays + l2l:
                assert L.lives_gpu_layer_pin(a) == 0
            s0 = stats(L)
            for i in range(n):
                tick_calls(L, wh, H, lays[i], l2l[i], mid, w, h, None, 40 + 13 * i, outpl, clamping)
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
        want = oracle_sink_track(orc, *srcs[i], w, h, mid, l2s[i], w, h, None, 40 + 13 * i, lut, outpl, clamping)
        same_planes(results[0][i][1], want, "track %d deferred / oracle" % i)
    return d


@pytest.mark.parametrize("n", [3, 16])
@pytest.mark.parametrize("outpl,mid,clamping", SINK_CASES, ids=["uyvy", "yuv420p", "yvu420p", "yuyv"])
def test_flat_sink_group_is_one_launch(seam, orc, deferred, flat, outpl, mid, clamping, n):
    """"no resize" followed by a YUV sink with the route on: ONE launch which is the chain launch [1], the sink launch [9], fused [11] and flat [13], carrying n tracks;
    no conversion pre-launch [7], not the 2:1 forms [5] / [12]; planes and leaves equal across deferred, eager and the oracle"""
    L, wh, H = seam
    assert flat(1) == 0
    d = sink_group(L, wh, H, orc, outpl, mid, clamping, n, 0xF5 + outpl + n)
    assert (d[4], d[8]) == (n, n), "every conversion was recorded, at both ends: %s" % d
    if FLAT_SINK[outpl]:
        assert (d[1], d[9], d[11], d[13]) == (1, 1, 1, 1) and (d[2], d[10], d[14]) == (n, n, n), "ONE lgpu_chain_flat_yuv420p_to_yuv launch with %d tracks: %s" % (n, d)
        assert (d[3], d[5], d[7], d[12]) == (0, 0, 0, 0), d
    else:
        assert (d[1], d[7], d[9], d[11], d[13], d[3]) == (1, 0, 1, 0, 1, 0), "lgpu_chain_flat_yuv420p into RGBA frames, then one batched conversion: %s" % d


def test_route_off_keeps_todays_launches(seam, orc, deferred, flat):
    """with the setter at 0 (the default) the counters are exactly today's: the conversion batch [7] and the chain [1] for the RGBA shapes, those two and one batched
    sink conversion [9] for the sink; [13] and [14] stay 0"""
    L, wh, H = seam
    n = 3
    for shape in RGBA_SHAPES:
        d, results, wants = rgba_group(L, wh, H, orc, shape, n, 0xF7)
        assert (d[1], d[2], d[3], d[5], d[7], d[13], d[14]) == (1, n, 0, 0, 1, 0, 0), "%s: %s" % (shape[-1], d)
        check_rgba(results, wants)
    d = sink_group(L, wh, H, orc, UYVY, RGBA32, CLAMPED, n, 0xF8)
    assert (d[1], d[3], d[5], d[7], d[9], d[10], d[11], d[12], d[13], d[14]) == (1, 0, 0, 1, 1, n, 0, 0, 0, 0), d


def test_seam_staged_wins(seam, orc, deferred, flat, tune):
    """SEAM_STAGED with the route on: no flat launch, no chain launch, every program walked stage by stage, the oracle's bytes"""
    L, wh, H = seam
    assert flat(1) == 0
    tune("SEAM_STAGED", 1)
    n = 3
    for shape in RGBA_SHAPES:
        d, results, wants = rgba_group(L, wh, H, orc, shape, n, 0xF9)
        assert (d[1], d[3], d[5], d[7], d[13], d[14]) == (0, n, 0, 0, 0, 0), "%s: %s" % (shape[-1], d)
        check_rgba(results, wants)
    d = sink_group(L, wh, H, orc, YUV420P, RGBA32, CLAMPED, n, 0xFA)
    assert (d[1], d[13], d[14], d[11]) == (0, 0, 0, 0) and d[3] == n, d
