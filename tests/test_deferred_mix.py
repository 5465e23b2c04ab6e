"""lives_gpu_set_pending_layer2: the second layer of a recorded "chroma blend" may stay a pending program.  A flush then FOLDS each reader and its layer 2 into ONE
lgpu_chain_flat_yuv_mix[_canvas] launch per 32 tracks -- the layer-2 programs stay pending and cost nothing unless somebody asks for their pixels -- or runs the layer-2
programs of the tick as a group of their own AHEAD of their readers (two launches whatever the shape).  Off (the default) every launch and counter is today's; SEAM_STAGED
still wins.  Compared three ways, as tests/test_deferred_flat.py does: deferred == eager (lives_gpu_set_deferred(0)) == the oracle's composition -- the oracle's conversion
of layer 2 (and its scale / letterbox) as `l2` of oracle_step, or of the sink's conversion behind it -- leaves included, for the readers and for the second layers."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.test_deferred import deferred, oracle_step, plan_step, seam, srgb_to  # noqa: F401 (fixtures)
from tests.test_deferred_flat import flat  # noqa: F401 (fixture)
from tests.test_deferred_flat422 import oracle_conv as oracle_conv422
from tests.test_deferred_flat422 import src_layer, src_planes
from tests.test_deferred_transcode import K4_FMT, equal_states, same_planes, state
from tests.test_deferred_yuv import yuv_layer, yuv_planes

needs_ref = pytest.mark.skipif(not po.have_ref(), reason="oracle/_ref (reference libweed) not built")
pytestmark = [needs_ref, pytest.mark.gpu]
P = po.P
RGBA32, BGRA32, YUV420P, YVU420P, YUV422P, UYVY, YUYV = 3, 4, 512, 513, 522, 564, 565
CLAMPED, UNCLAMPED = 0, 1
NSTATS = 19
W, H_ = 128, 72
NAMES = {YUV420P: "yuv420p", YVU420P: "yvu420p", YUV422P: "yuv422p", UYVY: "uyvy", YUYV: "yuyv", None: "rgba"}
# mode 1's rule (seam_lazy.cpp, MIX_FOLD_PAIRS): the pairs (layer 1, layer 2, letterboxed) whose one launch tools/bench_seam_transition.py shows ahead of mode 3's two
# launches by more than the latter's round-to-round spread.  profiles/r17/seam_transition.md (16 x 1080p, five interleaved rounds, us per tick, one launch against two
# and the two launches' spread): YUV420P over YUV420P 548.1 / 557.3 (123.4), UYVY over YUV420P 524.4 / 542.0 (18.4), YUV420P over UYVY 530.9 / 530.2 (7.0), YUV422P over
# YUV422P 589.5 / 584.8 (20.1), letterboxed YUV420P over YUV420P 618.4 / 635.2 (28.8): no pair is ahead by more than the spread, so none is folded; the pairs not timed
# are not folded either
MODE1_FOLDS = {(YUV420P, YUV420P, False): False, (YVU420P, YUV420P, False): False, (YUV420P, UYVY, False): False, (UYVY, YUYV, False): False, (YUV422P, UYVY, False): False,
               (UYVY, YUV420P, False): False, (YUV422P, YUV422P, False): False, (YUV420P, YUV422P, False): False, (YUV420P, YUV420P, True): False, (YUV420P, UYVY, True): False}


def stats(L):
    L.lives_gpu_deferred_stats_n.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    L.lives_gpu_deferred_stats_n.restype = None
    a = (ctypes.c_ulonglong * NSTATS)()
    L.lives_gpu_deferred_stats_n(a, NSTATS)
    return list(a)


def delta(a, b):
    return [y - x for x, y in zip(a, b)]


@pytest.fixture()
def pend(seam):
    """set / restore lives_gpu_set_pending_layer2 around a test; 0 is the default"""
    L = seam[0]
    L.lives_gpu_set_pending_layer2.argtypes = [ctypes.c_int]
    L.lives_gpu_set_pending_layer2.restype = ctypes.c_int
    prev = L.lives_gpu_set_pending_layer2(0)
    try:
        assert prev == 0, "a blend's second layer is run when the blend is recorded, by default"
        yield L.lives_gpu_set_pending_layer2
    finally:
        L.lives_gpu_set_pending_layer2(0)


def planar420(pal):
    return pal in (YUV420P, YVU420P)


def draw(rng, pal, w, h):
    """a decoded w x h frame of `pal` with padded rows, planes in Y, U, V order"""
    return list(yuv_planes(rng, w, h, pad=(4, 2, 6))) if planar420(pal) else src_planes(rng, pal, w, h)


def make_layer(wh, pal, w, h, planes):
    return yuv_layer(wh, pal, w, h, *planes) if planar420(pal) else src_layer(wh, pal, w, h, planes)


def conv(orc, pal, planes, w, h, order):
    """the oracle's conversion of a decoded frame into a tight RGBA (order 0) / BGRA (order 1) frame"""
    if not planar420(pal):
        return oracle_conv422(orc, pal, planes, w, h, order)
    Y, U, V = planes
    rgba = np.zeros((h, w * 4), np.uint8)
    st = (ctypes.c_int * 3)(Y.strides[0], U.strides[0], V.strides[0])
    orc.orc_yuv420p_to_rgb(P(Y), P(U), P(V), st, U.size, V.size, P(rgba), w * 4, w, h, 4, order, 0, 0, 2, None, 0)
    return rgba


def spec(p1, p2, outpl=None, mid=RGBA32, s1=(W, H_), s2=None, d1=None, d2=None, cv1=None, cv2=None, clamping=CLAMPED, gamma=2):
    """one tick's shape: layer 1 of palette p1 and size s1 is converted to `mid`, resized to d1, [letterboxed onto cv1], blended with layer 2, gamma-converted and [handed
    to the sink palette outpl]; layer 2 of palette p2 and size s2 is converted to `mid`, resized to d2 and [letterboxed onto cv2] before it is blended"""
    s2 = s2 or s1
    d1 = d1 or s1
    return dict(p1=p1, p2=p2, outpl=outpl, mid=mid, s1=s1, s2=s2, d1=d1, d2=d2 or (d1 if s2 == s1 else s2), cv1=cv1, cv2=cv2, clamping=clamping, gamma=gamma)


def oracle_l2(orc, sp, planes):
    """layer 2 as the blend reads it"""
    order = 1 if sp["mid"] == BGRA32 else 0
    (sw, sh), (dw, dh) = sp["s2"], sp["d2"]
    return oracle_step(orc, conv(orc, sp["p2"], planes, sw, sh, order), sw, sh, None, dw, dh, sp["cv2"], 0, None, False)


def oracle_reader(orc, sp, planes, l2, bf):
    """one reader's planes: the RGBA frame, or the sink's planes in the layer's plane order"""
    order = 1 if sp["mid"] == BGRA32 else 0
    (sw, sh), (dw, dh) = sp["s1"], sp["d1"]
    lut = srgb_to(orc, sp["gamma"]) if sp["gamma"] is not None else None
    out = oracle_step(orc, conv(orc, sp["p1"], planes, sw, sh, order), sw, sh, l2, dw, dh, sp["cv1"], bf, lut, False)
    if sp["outpl"] is None:
        return [out]
    w, h = sp["cv1"] if sp["cv1"] else (dw, dh)
    fmt = K4_FMT[sp["outpl"]]
    if fmt == 4:
        w, h = w & ~1, h & ~1
    want, _ = po.k4_out_planes(0, w, h, fmt, 0)
    wp, ws = po.planes_args(want)
    assert orc.orc_rgb_to_yuv(P(out), out.strides[0], w, h, order, 1, ctypes.addressof(wp), ctypes.addressof(ws), fmt, 0, 1 if sp["clamping"] == UNCLAMPED else 0) == 0
    return [want[0], want[2], want[1]] if sp["outpl"] == YVU420P else want


def bf_of(i):
    return (40 + 13 * i) & 0xFF


def record(L, wh, H, sp, lays, l2l, reads):
    """the calls of a tick, track by track: layer 2's plan step without a blend or a gamma change, then the reader's"""
    for l2 in l2l:
        plan_step(L, wh, H, l2, None, sp["d2"][0], sp["d2"][1], sp["cv2"], 0, None, swap_to=sp["mid"])
    for i, lay in enumerate(lays):
        plan_step(L, wh, H, lay, l2l[reads[i]], sp["d1"][0], sp["d1"][1], sp["cv1"], bf_of(i), sp["gamma"], swap_to=sp["mid"])
        if sp["outpl"] is not None:
            assert L.lives_gpu_convert_layer_palette_full(lay, sp["outpl"], sp["clamping"], 0, 1, 2) == 1


def tick(L, wh, H, orc, sp, n, seed, m=None, middle=None, list_l2=False):
    """n readers over m second layers (reader i reads layer 2 number i % m; m = n by default), deferred and eager.  middle(L, lays, l2l): what happens between the
    recording and the end, instead of one flush of the readers (list_l2: of the second layers too).  Every layer is then synchronised, the readers first, and compared:
    deferred == eager == oracle.  Returns the deferred run's counter deltas: (up to the flush / the middle, from there to the readers' syncs, over the FIRST layer 2's
    sync, over the syncs of the others)"""
    m = m or n
    rng = np.random.default_rng(seed)
    srcs = [draw(rng, sp["p1"], *sp["s1"]) for _ in range(n)]
    l2srcs = [draw(rng, sp["p2"], *sp["s2"]) for _ in range(m)]
    reads = [i % m for i in range(n)]
    results, ds = [], None
    try:
        for mode in (1, 0):
            L.lives_gpu_set_deferred(mode)
            lays = [make_layer(wh, sp["p1"], *sp["s1"], srcs[i]) for i in range(n)]
            l2l = [make_layer(wh, sp["p2"], *sp["s2"], l2srcs[j]) for j in range(m)]
            for a in lays + l2l:
                assert L.lives_gpu_layer_pin(a) == 0
            s0 = stats(L)
            record(L, wh, H, sp, lays, l2l, reads)
            if middle is not None:
                middle(L, lays, l2l)
            else:
                listed = lays + (l2l if list_l2 else [])
                assert L.lives_gpu_layers_flush((ctypes.c_void_p * len(listed))(*listed), len(listed)) == 0
            s1 = stats(L)
            out = []
            for a in lays:
                assert L.lives_gpu_layer_sync(a) == 0
                out.append(state(wh, a))
            s2 = stats(L)
            assert L.lives_gpu_layer_sync(l2l[0]) == 0
            s3 = stats(L)
            out2 = []
            for a in l2l:
                assert L.lives_gpu_layer_sync(a) == 0
                out2.append(state(wh, a))
            s4 = stats(L)
            if mode:
                ds = (delta(s0, s1), delta(s1, s2), delta(s2, s3), delta(s3, s4))
            else:
                assert delta(s0, s4) == [0] * NSTATS, "the eager run records and launches nothing deferred"
            results.append((out, out2))
            for a in lays + l2l:
                assert L.lives_gpu_layer_unpin(a) == 0
    finally:
        L.lives_gpu_set_deferred(1)
    for j in range(m):
        equal_states(results[0][1][j], results[1][1][j], "layer 2 number %d deferred / eager" % j)
    wants2 = [oracle_l2(orc, sp, l2srcs[j]) for j in range(m)]
    for j in range(m):
        same_planes(results[0][1][j][1], [wants2[j]], "layer 2 number %d deferred / oracle" % j)
    for i in range(n):
        equal_states(results[0][0][i], results[1][0][i], "track %d deferred / eager" % i)
        same_planes(results[0][0][i][1], oracle_reader(orc, sp, srcs[i], wants2[reads[i]], bf_of(i)), "track %d deferred / oracle" % i)
    return ds


def check_folded(ds, n, sink, nl2=None, l2_canvas=False):
    """ONE mix launch per 32 tracks and nothing else; a layer 2 stays pending until its pixels are asked for, and its conversion is then one batch of one (letterboxed:
    one flat launch of one track)"""
    d, d_sync, d_l2, _ = ds
    nl2 = n if nl2 is None else nl2
    launches = (n + 31) // 32
    assert d[4] == n + nl2 and d[15] == n, "both conversions of every track were recorded, every blend against a pending layer 2: %s" % d
    assert (d[1], d[13], d[16]) == (launches,) * 3 and (d[2], d[14], d[17]) == (n,) * 3, "%d lgpu_chain_flat_yuv_mix launch(es) with %d tracks: %s" % (launches, n, d)
    assert (d[3], d[5], d[7], d[18]) == (0, 0, 0, 0), d
    assert (d[9], d[11]) == ((launches, launches) if sink else (0, 0)), d
    assert d_sync == [0] * NSTATS, "the readers' syncs ran nothing more: %s" % d_sync
    assert (d_l2[7], d_l2[1], d_l2[13]) == ((0, 1, 1) if l2_canvas else (1, 0, 0)) and (d_l2[16], d_l2[18]) == (0, 0), "a later sync of a layer 2 runs its program, alone: %s" % d_l2


def check_l2_first(ds, n, nl2=None):
    d, d_sync, d_l2, d_rest = ds
    nl2 = n if nl2 is None else nl2
    assert d[15] == n and d[18] == nl2 and (d[16], d[17]) == (0, 0), "every layer-2 program ran ahead of its readers, nothing was folded: %s" % d
    assert d_sync == [0] * NSTATS and d_l2 == [0] * NSTATS and d_rest == [0] * NSTATS, "the syncs ran nothing more"


FOLD_PAIRS = [(YUV420P, YUV420P), (YVU420P, YUV420P), (YUV420P, UYVY), (UYVY, YUYV), (YUV422P, UYVY)]
DESTS = [(None, RGBA32, CLAMPED), (UYVY, BGRA32, CLAMPED), (YUV420P, RGBA32, UNCLAMPED)]


def pair_ids(pairs):
    return ["l1-%s_l2-%s" % (NAMES[a], NAMES[b]) for a, b in pairs]


@pytest.mark.parametrize("n", [1, 3, 16])
@pytest.mark.parametrize("outpl,mid,clamping", DESTS, ids=["to_rgba", "to_uyvy", "to_yuv420p"])
@pytest.mark.parametrize("pair", FOLD_PAIRS, ids=pair_ids(FOLD_PAIRS))
def test_folded_tick_is_one_launch(seam, orc, deferred, flat, pend, pair, outpl, mid, clamping, n):
    """mode 2, two decoded layers of the project's size per track: convert -> chroma blend -> gamma [-> sink] of n tracks is ONE lgpu_chain_flat_yuv_mix launch"""
    L, wh, H = seam
    assert flat(1) == 0 and pend(2) == 0
    ds = tick(L, wh, H, orc, spec(pair[0], pair[1], outpl, mid, clamping=clamping), n, [0x3A1, pair[0], pair[1], outpl or 0, n])
    check_folded(ds, n, outpl is not None)


@pytest.mark.parametrize("outpl,mid,clamping", [DESTS[0], DESTS[2]], ids=["to_rgba", "to_yuv420p"])
def test_folded_tick_of_33_tracks_is_two_launches(seam, orc, deferred, flat, pend, outpl, mid, clamping):
    L, wh, H = seam
    assert flat(1) == 0 and pend(2) == 0
    check_folded(tick(L, wh, H, orc, spec(YUV420P, YUV420P, outpl, mid, clamping=clamping), 33, [0x3A2, outpl or 0]), 33, outpl is not None)


def test_listed_second_layers_stay_pending_when_folded(seam, orc, deferred, flat, pend):
    """the second layers are handed to the flush with their readers: the same one launch, and their programs are still pending afterwards"""
    L, wh, H = seam
    assert flat(1) == 0 and pend(2) == 0
    check_folded(tick(L, wh, H, orc, spec(YUV420P, UYVY), 3, 0x3A3, list_l2=True), 3, False)


L2_FIRST_PAIRS = [(UYVY, YUV420P), (YUV422P, YUV422P), (YUV420P, YUV420P)]


@pytest.mark.parametrize("n", [3, 16])
@pytest.mark.parametrize("pair", L2_FIRST_PAIRS, ids=pair_ids(L2_FIRST_PAIRS))
def test_mode_3_runs_the_second_layers_first(seam, orc, deferred, flat, pend, pair, n):
    """mode 3 never folds: ONE batched conversion [7] serves all the second layers, ONE flat launch [13] their readers -- two launches for the tick"""
    L, wh, H = seam
    assert flat(1) == 0 and pend(3) == 0
    ds = tick(L, wh, H, orc, spec(*pair), n, [0x3A4, pair[0], pair[1], n])
    check_l2_first(ds, n)
    d = ds[0]
    assert (d[7], d[1], d[2], d[13], d[14], d[3], d[5]) == (1, 1, n, 1, n, 0, 0), d


def test_mode_2_without_the_flat_route_runs_the_second_layers_first(seam, orc, deferred, flat, pend):
    """folding needs lives_gpu_set_flat_yuv(1): without it the second layers' batched conversion [7], then today's two launches of the readers ([7] again, [1])"""
    L, wh, H = seam
    assert pend(2) == 0
    n = 3
    ds = tick(L, wh, H, orc, spec(YUV420P, YUV420P), n, 0x3A5)
    check_l2_first(ds, n)
    d = ds[0]
    assert (d[7], d[1], d[2], d[13], d[3]) == (2, 1, n, 0, 0), d


def test_a_second_layer_with_a_stage_of_its_own_runs_first(seam, orc, deferred, flat, pend):
    """layer 2 converted to BGRA32 and then swapped to RGBA32 is a program of two stages, converted into the other byte order than the blend works in: more than the
    conversion the mix form reads, so it runs ahead of its readers"""
    L, wh, H = seam
    assert flat(1) == 0 and pend(2) == 0
    n = 2
    rng = np.random.default_rng(0x3A6)
    srcs, l2srcs = [draw(rng, YUV420P, W, H_) for _ in range(n)], [draw(rng, YUV420P, W, H_) for _ in range(n)]
    lays, l2l = [make_layer(wh, YUV420P, W, H_, s) for s in srcs], [make_layer(wh, YUV420P, W, H_, s) for s in l2srcs]
    for a in lays + l2l:
        assert L.lives_gpu_layer_pin(a) == 0
    s0 = stats(L)
    for a in l2l:
        assert L.lives_gpu_convert_layer_palette(a, BGRA32, 0) == 1 and L.lives_gpu_convert_layer_palette(a, RGBA32, 0) == 1
    for i, a in enumerate(lays):
        plan_step(L, wh, H, a, l2l[i], W, H_, None, bf_of(i), 2)
    assert L.lives_gpu_layers_flush((ctypes.c_void_p * n)(*lays), n) == 0
    d = delta(s0, stats(L))
    assert d[15] == n and d[18] == n and d[16] == 0, d
    lut = srgb_to(orc, 2)
    for i, a in enumerate(lays):
        assert L.lives_gpu_layer_sync(a) == 0
        l2 = conv(orc, YUV420P, l2srcs[i], W, H_, 1)
        l2s = np.zeros_like(l2)
        orc.orc_swizzle(po.OPS.index("swap3postalpha"), 0, P(l2), W * 4, P(l2s), W * 4, W, H_, None)
        want = oracle_step(orc, conv(orc, YUV420P, srcs[i], W, H_, 0), W, H_, l2s, W, H_, None, bf_of(i), lut, False)
        same_planes(state(wh, a)[1], [want], "track %d" % i)
    for a in lays + l2l:
        assert L.lives_gpu_layer_unpin(a) == 0


def test_scaled_layers_take_two_2_to_1_launches(seam, orc, deferred, flat, pend):
    """both layers 256 x 144 -> 128 x 72 from YUV420P, mode 2: nothing to fold -- the second layers as ONE lgpu_chain_yuv420p launch without a blend, then their readers
    as another"""
    L, wh, H = seam
    assert flat(1) == 0 and pend(2) == 0
    n = 3
    ds = tick(L, wh, H, orc, spec(YUV420P, YUV420P, s1=(256, 144), d1=(W, H_), d2=(W, H_)), n, 0x3A7)
    check_l2_first(ds, n)
    d = ds[0]
    assert (d[5], d[6], d[1], d[2], d[7], d[13], d[3]) == (2, 2 * n, 2, 2 * n, 0, 0, 0), d


@pytest.mark.parametrize("pair", [(YUV420P, YUV420P), (YUV422P, UYVY)], ids=pair_ids([(YUV420P, YUV420P), (YUV422P, UYVY)]))
def test_letterboxed_onto_one_canvas_is_one_launch(seam, orc, deferred, flat, pend, pair):
    """both layers 128 x 72 letterboxed onto (160, 100): ONE lgpu_chain_flat_yuv_mix_canvas launch, bars included"""
    L, wh, H = seam
    assert flat(1) == 0 and pend(2) == 0
    n = 3
    check_folded(tick(L, wh, H, orc, spec(pair[0], pair[1], cv1=(160, 100), cv2=(160, 100)), n, [0x3A8, pair[0], pair[1]]), n, False, l2_canvas=True)


def test_letterboxes_that_differ_run_the_second_layers_first(seam, orc, deferred, flat, pend):
    """a second layer that fills the canvas by itself (a letterbox on layer 1 only), and one letterboxed from another frame size (another place on the canvas)"""
    L, wh, H = seam
    assert flat(1) == 0 and pend(2) == 0
    n = 3
    for k, sp in enumerate([spec(YUV420P, YUV420P, cv1=(160, 100), s2=(160, 100)), spec(YUV420P, UYVY, cv1=(160, 100), s2=(120, 72), cv2=(160, 100))]):
        ds = tick(L, wh, H, orc, sp, n, [0x3A9, k])
        check_l2_first(ds, n)
        assert ds[0][3] == 0, ds[0]


MODE1_CASES = sorted(MODE1_FOLDS, key=str)


@pytest.mark.parametrize("case", MODE1_CASES, ids=["l1-%s_l2-%s%s" % (NAMES[a], NAMES[b], "_canvas" if c else "") for a, b, c in MODE1_CASES])
def test_mode_1_folds_the_pairs_on_file(seam, orc, deferred, flat, pend, case):
    """mode 1 folds what MODE1_FOLDS names and runs the second layers first for every other pair; the same ticks fold under mode 2, so the case shows the rule and not
    a shape the fold cannot take"""
    L, wh, H = seam
    assert flat(1) == 0 and pend(1) == 0
    p1, p2, canvas = case
    n = 3
    cv = (160, 100) if canvas else None
    ds = tick(L, wh, H, orc, spec(p1, p2, cv1=cv, cv2=cv), n, [0x3AA, p1, p2, int(canvas)])
    if MODE1_FOLDS[case]:
        check_folded(ds, n, False, l2_canvas=canvas)
    else:
        check_l2_first(ds, n)
    assert pend(2) == 1
    check_folded(tick(L, wh, H, orc, spec(p1, p2, cv1=cv, cv2=cv), n, [0x3AA, p1, p2, int(canvas)]), n, False, l2_canvas=canvas)


def test_mode_0_is_todays_tick(seam, orc, deferred, flat, pend):
    """off: the counters [0..14] of the same ticks are those of a process that never called the setter -- every second layer runs alone when its blend is recorded
    ([7] == n), then ONE flat launch -- and [15..18] stay 0; the same after the setter has been on and is off again"""
    L, wh, H = seam
    assert flat(1) == 0
    n = 3
    seen = []
    for k in range(2):
        for sp in (spec(YUV420P, YUV420P), spec(YUV422P, UYVY, UYVY, BGRA32), spec(YUV420P, YUV420P, cv1=(160, 100), cv2=(160, 100))):
            ds = tick(L, wh, H, orc, sp, n, [0x3AB, sp["p1"]])
            d = ds[0]
            assert d[15:] == [0, 0, 0, 0] and [x[15:] for x in ds[1:]] == [[0, 0, 0, 0]] * 3, ds
            assert d[4] == 2 * n and d[3] == 0, d
            # every second layer ran alone when its blend was recorded -- a conversion as a batch of one [7], a letterboxed one as a flat launch of one track [13] --
            # and the readers share one flat launch
            assert (d[7], d[13]) == ((n, 1) if sp["cv2"] is None else (0, n + 1)), d
            seen.append([x[:15] for x in ds])
        assert pend(2) == 0 and pend(0) == 2
    assert seen[:3] == seen[3:]


def test_one_second_layer_read_by_two_tracks(seam, orc, deferred, flat, pend):
    """two readers of ONE pending layer 2: folded, its planes ride in both tracks of the one launch; run first, it runs once"""
    L, wh, H = seam
    assert flat(1) == 0 and pend(2) == 0
    check_folded(tick(L, wh, H, orc, spec(YUV420P, YUV420P), 2, 0x3AC, m=1), 2, False, nl2=1)
    check_folded(tick(L, wh, H, orc, spec(UYVY, YUYV, YUV420P, RGBA32), 4, 0x3AD, m=2), 4, True, nl2=2)
    assert pend(3) == 2
    check_l2_first(tick(L, wh, H, orc, spec(YUV420P, YUV420P), 2, 0x3AE, m=1), 2, nl2=1)


def test_whoever_needs_the_pixels_first_gets_them(seam, orc, deferred, flat, pend):
    """without a flush: a sync of a reader folds it alone; a sync of layer 2 runs it and the reader then reads the plane; a gamma pass on layer 2 after the blend was
    recorded, and its unpinning, run layer 2 and then its readers first -- always the bytes of the eager run, for the readers and for layer 2 (tick() compares both)"""
    L, wh, H = seam
    assert flat(1) == 0 and pend(2) == 0
    n = 2
    sp = spec(YUV420P, UYVY)

    def nothing(L_, lays, l2l):
        pass
    ds = tick(L, wh, H, orc, sp, n, 0x3B0, middle=nothing)
    assert ds[0][15] == n and ds[0][1] == 0, "nothing has run yet: %s" % ds[0]
    assert (ds[1][16], ds[1][17], ds[1][1], ds[1][18], ds[1][7]) == (n, n, n, 0, 0), "each reader's sync is a mix launch of one track: %s" % ds[1]
    assert ds[2][7] == 1, ds[2]

    def sync_l2_first(L_, lays, l2l):
        for a in l2l:
            assert L_.lives_gpu_layer_sync(a) == 0
    ds = tick(L, wh, H, orc, sp, n, 0x3B1, middle=sync_l2_first)
    assert ds[0][15] == n and ds[0][7] == n and ds[0][1] == 0, "the second layers ran, one by one; their readers did not: %s" % ds[0]
    assert (ds[1][13], ds[1][16], ds[1][18]) == (n, 0, 0), "the readers read resident planes: %s" % ds[1]


def test_a_change_of_layer_2_runs_it_and_its_readers_first(seam, orc, deferred, flat, pend):
    """gamma_convert_layer on layer 2 after the blend was recorded, then unpinning it with a reader pending: the reader sees layer 2 as it was when the blend was called,
    and layer 2 comes home with the gamma pass on it.  Then layer 2 has no readers left: observable as a stage being recorded on a fresh pending layer 2 again"""
    L, wh, H = seam
    assert flat(1) == 0
    rng = np.random.default_rng(0x3B2)
    src, l2src, l2bsrc = draw(rng, YUV420P, W, H_), draw(rng, YUV420P, W, H_), draw(rng, UYVY, W, H_)
    lut = srgb_to(orc, 2)
    outs = []
    for mode, pmode in ((1, 2), (1, 3), (0, 0)):
        L.lives_gpu_set_deferred(mode)
        pend(pmode)
        lay, l2, l2b = make_layer(wh, YUV420P, W, H_, src), make_layer(wh, YUV420P, W, H_, l2src), make_layer(wh, UYVY, W, H_, l2bsrc)
        for a in (lay, l2, l2b):
            assert L.lives_gpu_layer_pin(a) == 0
        assert L.lives_gpu_convert_layer_palette(l2, RGBA32, 0) == 1
        plan_step(L, wh, H, lay, l2, W, H_, None, 140, None)
        s0 = stats(L)
        assert L.lives_gpu_gamma_convert_layer(2, l2) == 1                     # changes layer 2 AFTER the blend was called
        d = delta(s0, stats(L))
        if mode:
            assert d[0] == 0 and d[7] == 1 and d[1] == 1, "layer 2 ran, then its reader, and the gamma pass was not recorded on a plane with readers: %s" % d
        assert L.lives_gpu_layer_unpin(l2) == 0
        assert L.lives_gpu_layer_sync(lay) == 0
        outs.append((state(wh, lay), state(wh, l2)))
        # a second blend, against another pending layer 2, which is unpinned with the reader pending
        assert L.lives_gpu_layer_unpin(lay) == 0
        lay = make_layer(wh, YUV420P, W, H_, src)
        assert L.lives_gpu_layer_pin(lay) == 0
        assert L.lives_gpu_convert_layer_palette(l2b, RGBA32, 0) == 1
        plan_step(L, wh, H, lay, l2b, W, H_, None, 77, 2)
        s0 = stats(L)
        assert L.lives_gpu_layer_unpin(l2b) == 0
        d = delta(s0, stats(L))
        if mode:
            assert d[7] == 1 and d[1] == 1 and d[13] == 1 and d[16] == 0, "layer 2 came home first, then its reader ran on the plane: %s" % d
        assert L.lives_gpu_layer_sync(lay) == 0
        outs[-1] += (state(wh, lay), state(wh, l2b))
        assert L.lives_gpu_layer_unpin(lay) == 0
    L.lives_gpu_set_deferred(1)
    for k in (0, 1):
        for a, b in zip(outs[k], outs[2]):
            equal_states(a, b, "deferred (run %d) / eager" % k)
    l2_then = conv(orc, YUV420P, l2src, W, H_, 0)
    same_planes(outs[0][0][1], [oracle_step(orc, conv(orc, YUV420P, src, W, H_, 0), W, H_, l2_then, W, H_, None, 140, None, False)], "reader")
    l2_now = l2_then.copy()
    orc.orc_gamma_apply(P(l2_now), W * 4, W, H_, 4, 0, P(lut))
    same_planes(outs[0][1][1], [l2_now], "layer 2")
    l2b_then = conv(orc, UYVY, l2bsrc, W, H_, 0)
    same_planes(outs[0][2][1], [oracle_step(orc, conv(orc, YUV420P, src, W, H_, 0), W, H_, l2b_then, W, H_, None, 77, lut, False)], "second reader")
    same_planes(outs[0][3][1], [l2b_then], "second layer 2")


def test_a_reader_that_is_dropped_runs_nothing_and_lets_go_of_layer_2(seam, orc, deferred, flat, pend):
    """a reader that is forgotten before it ever ran: nothing runs, and layer 2 has no reader left -- the next stage on it is RECORDED again (with a reader it would run
    layer 2 and the reader first).  A reader that is unpinned instead comes home with the eager run's bytes, folded alone, and lets go of layer 2 as well"""
    L, wh, H = seam
    assert flat(1) == 0 and pend(2) == 0
    rng = np.random.default_rng(0x3B3)
    src, l2src = draw(rng, YUV420P, W, H_), draw(rng, YUV422P, W, H_)
    lut = srgb_to(orc, 2)
    for how in ("forget", "unpin"):
        lay, l2 = make_layer(wh, YUV420P, W, H_, src), make_layer(wh, YUV422P, W, H_, l2src)
        assert L.lives_gpu_layer_pin(lay) == 0 and L.lives_gpu_layer_pin(l2) == 0
        assert L.lives_gpu_convert_layer_palette(l2, RGBA32, 0) == 1
        plan_step(L, wh, H, lay, l2, W, H_, None, 99, 2)
        s0 = stats(L)
        if how == "forget":
            assert L.lives_gpu_layer_forget(lay) == 0
            assert delta(s0, stats(L)) == [0] * NSTATS, "nothing ran for the dropped reader"
        else:
            assert L.lives_gpu_layer_unpin(lay) == 0
            d = delta(s0, stats(L))
            assert (d[16], d[17], d[7], d[18]) == (1, 1, 0, 0), d
            l2_then = conv(orc, YUV422P, l2src, W, H_, 0)
            same_planes(state(wh, lay)[1], [oracle_step(orc, conv(orc, YUV420P, src, W, H_, 0), W, H_, l2_then, W, H_, None, 99, lut, False)], "the unpinned reader")
        s0 = stats(L)
        assert L.lives_gpu_gamma_convert_layer(2, l2) == 1
        d = delta(s0, stats(L))
        assert d[0] == 1 and d[1:] == [0] * (NSTATS - 1), "the gamma pass was recorded on layer 2's program, which is still pending and has no reader: %s" % d
        assert L.lives_gpu_layer_unpin(l2) == 0
        want = conv(orc, YUV422P, l2src, W, H_, 0)
        orc.orc_gamma_apply(P(want), W * 4, W, H_, 4, 0, P(lut))
        same_planes(state(wh, l2)[1], [want], "layer 2")


def test_seam_staged_wins_over_every_mode(seam, orc, deferred, flat, pend, tune):
    """SEAM_STAGED with the route on, in every mode: no mix launch, no chain launch; the second layers run first (mode 0: when recorded), one conversion each, and every
    reader is walked stage by stage; the oracle's bytes"""
    L, wh, H = seam
    assert flat(1) == 0
    tune("SEAM_STAGED", 1)
    n = 3
    for mode in (2, 1, 3, 0):
        pend(mode)
        ds = tick(L, wh, H, orc, spec(YUV420P, YUV420P), n, [0x3B4, mode])
        d = ds[0]
        assert (d[1], d[13], d[16], d[17], d[3]) == (0, 0, 0, 0, n), "mode %d: %s" % (mode, d)
        assert d[18] == (n if mode else 0) and d[15] == (n if mode else 0), "mode %d: %s" % (mode, d)
