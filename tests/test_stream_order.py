"""Every frame-level entry point on a busy non-default stream: the bytes of the oracle after synchronising THAT stream only, and a return while the stream is busy.

include/lives_gpu.h: "Every entry point below takes a `stream`"; the layer seam gives each host thread a non-blocking stream of its own.  The other suites call on
the null stream and download behind a device-wide synchronize, so a launch on the wrong stream, a table copied on the null stream or a scratch stage enqueued
somewhere else passes them by construction, and so does a hidden hipStreamSynchronize / hipDeviceSynchronize / blocking hipMemcpy / hipFree in a steady-state call,
which would serialise the host's threads.  tests/stream_order.py:StreamProxy stands where the existing runners expect `gpu` (its docstring has the six steps); the
runners' own comparisons with the oracle are the byte check, the proxy's event query is the "did not wait" check.

  teeth       the harness catches a stray launch, a stray first stage and a wait, with torch ops only
  inventory   every prototype of the header with a `void *stream` is in SWEPT (name -> the cases that call it; the GPU sweep checks that they really do) or EXEMPT
  sweep       tests/test_address_alignment.py's groups (for each, the first class that reaches each planned form, refusals left out), the tick forms' own runners
              at their multi-launch shapes, the runtime's copies and fills; one test per runner (BUNDLES), every case with a proxy of its own
  sequences   Blurzoom / RgbDelay: seven frames behind ONE busy period, no host synchronisation between them
  back to back  two calls with different inputs AND parameters behind one busy period: staging memory and kernel arguments of the first must have left before the second
  cold start  one fresh child process makes its first ever call of every lazily initialising path on a busy side stream

EXPECTED_WAITS lists the calls that are allowed to wait for their stream once warm -- and then must: a listed call that does not wait fails too.
"""
import collections
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import stream_order as so
from tests import test_address_alignment as aa
from tests.util import align, frame

G = pytest.mark.gpu
P = po.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "lives_gpu.h")) as _f:
    STREAM_NAMES = so.stream_entry_points(_f.read())

# ---------------------------------------------------------------------------------------------- the inventory
# the prototypes that are not swept, each with its reason
EXEMPT = {
    "lgpu_malloc_ordered": "the runtime's own allocator: tests/test_gpu_parity.py:test_stream_ordered_allocation orders it against a stream",
    "lgpu_free_ordered": "as lgpu_malloc_ordered",
    "lgpu_stream_destroy": "takes the stream as its object, enqueues nothing",
    "lgpu_event_record": "the runtime's own event calls: test_stream_and_event_entry_points",
    "lgpu_stream_wait_event": "as lgpu_event_record",
    "lgpu_sync": "exists to wait",
    "lgpu_stream_query": "enqueues nothing",
    "lgpu_download": "writes host memory and is complete only after lgpu_sync(stream): there is no device result to hold against the oracle",
    "lgpu_pixbuf_scale_check": "does no device work (it answers from the planner)",
    "lgpu_chain_timed": "exists to wait: it times `reps` launches with events and returns the milliseconds",
    "lgpu_debug_stream_probe": "as lgpu_chain_timed, and leaves its destinations dirty",
    "lgpu_params_broadcast": "needs an RCCL communicator: tests/test_stepper.py",
    "lgpu_params_broadcast_n": "needs an RCCL communicator: tests/test_stepper.py",
    "lgpu_status_allreduce": "needs an RCCL communicator: tests/test_stepper.py",
    "lgpu_fan_in": "needs an RCCL communicator: tests/test_stepper.py",
}

# the calls that wait for their stream after the warm-up: case -> {index of the judged call: (entry point, source line that waits, what allows it)}
EXPECTED_WAITS = {
    "seq:rgbdelay-tables": {1: ("RgbDelay.process", "stencil.hip: if (s->in_flight) hipEventSynchronize(s->copied)",
                                "more than four jobs travel through ONE pinned staging table per handle; the second upload waits until the first has left it")},
    "seq:rgbdelay-ring": {3: ("RgbDelay.process", "stencil.hip: if (maxneeded != s->tcache) hipStreamSynchronize(st)",
                              "the ring of frames inside the handle is resized (hipMalloc / hipFree) when the parameters ask for another depth: scratch growth")},
    "b2b:upload": {1: ("lgpu_upload", "runtime.hip: if (t_stage.busy[k]) hipEventSynchronize(t_stage.ev[k])",
                       "lives_gpu.h: pageable uploads go through two pinned staging chunks per host thread; a chunk is reused when its DMA has finished")},
}


def expect_wait(cid):
    listed = EXPECTED_WAITS.get(cid, {})
    return lambda name, index: index in listed and listed[index][0] == name


# ---------------------------------------------------------------------------------------------- the cases
CASES = collections.OrderedDict()          # id -> fn(px, orc, tune); px None: the dry pass (inputs, oracle and argument binding, no device)
STATEFUL_RUNNERS = (aa.run_rgbdelay, aa.run_blurzoom)      # two frames through one handle: a warm-up of the call would advance it.  The sequences below stand for them


def case(cid):
    def reg(fn):
        assert cid not in CASES
        CASES[cid] = fn
        return fn
    return reg


class StreamStage(aa.Stage):
    """tests/test_address_alignment.py's Stage whose buffers are recorded by the proxy as they are uploaded: the runners hand some entry points raw pointers
    (gpu.lib.call), which carry no tensor"""

    def dev(self, name):
        t = super().dev(name)
        self.gpu.record(t)
        return t


def chosen_classes(orc, grp):
    """for one group, the first class that reaches each distinct planned form; refusals (LGPU_E_BADARG / LGPU_E_UNSUPPORTED classes) are left out"""
    gid, run, params, cls, expect, forms = grp
    seen, out = set(), []
    for label, place in cls:
        plan = aa.Stage(None, place)
        planned = run(orc, plan, *params)
        plan.finish()
        if planned in aa.CODES or planned in seen:
            continue
        seen.add(planned)
        out.append((label, place, planned))
    return out


def group_case(grp):
    def fn(px, orc, tune):
        gid, run, params = grp[:3]
        chosen = chosen_classes(orc, grp)
        assert chosen, "%s: no class to run" % gid
        for label, place, planned in chosen:
            if px is None:
                continue
            st = StreamStage(px, place, tune)
            try:
                actual = run(orc, st, *params)
            except AssertionError as e:
                raise AssertionError("%s, class %s (%s) on a busy side stream: %s" % (gid, label, planned, e)) from None
            assert actual == planned, (gid, label, actual, planned)
    return fn


for _grp in aa.GROUPS:
    if _grp[1] not in STATEFUL_RUNNERS:
        CASES["grp:" + _grp[0]] = group_case(_grp)


def tick(px, orc, runner, *args, **kw):
    """one of the tick forms' own runners (they upload for themselves, so there is no oracle-only mode): dry, the arguments are bound to the runner's signature"""
    if px is None:
        inspect.signature(runner).bind(None, orc, *args, **kw)
        return
    runner(px, orc, *args, **kw)


def lut_of(orc):
    from tests.test_chain_flat import gamma_lut
    return gamma_lut(orc)


@case("tick:chain_yuv420p-canvas")
def _(px, orc, tune):
    """lgpu_chain_yuv420p onto a letterbox canvas: bars plus frame"""
    from tests.test_chain_yuv import run
    tick(px, orc, run, np.random.default_rng(0x5701), 132, 76, ntracks=2, blend=True, lut=lut_of(orc), canvas=True, wt=1, pad=(3, 5, 1), tight=True)


@case("tick:chain_to_yuv-33")
def _(px, orc, tune):
    from tests.test_chain_sink import run
    tick(px, orc, run, np.random.default_rng(0x5702), 16, 12, 4, ntracks=33, blend=True, lut=lut_of(orc), wt=2, in_order=1, swap=1, yvu=True, pads=(4, 8, 0))


for _n in (33, 64):
    @case("tick:transcode-%d-yuv420p" % _n)
    def _(px, orc, tune, n=_n):
        """lgpu_chain_yuv420p_to_yuv: LGPU_CHAIN_TRANSCODE_TRACKS tracks per launch, so two launches"""
        from tests.test_chain_transcode import run
        tick(px, orc, run, np.random.default_rng(0x5703 + n), 16, 12, 4, ntracks=n, blend=True, lut=lut_of(orc), order=1, wt_src=2, wt_sink=2, yvu_sink=True, pad=(4, 0, 2), pads=(4, 8, 0))

    @case("tick:flat-%d-yuv420p" % _n)
    def _(px, orc, tune, n=_n):
        """lgpu_chain_flat_yuv420p_to_yuv to the 4:2:0 sink: kFlatPlanarTracks = 32 tracks per launch, so two launches"""
        from tests.test_chain_flat import run
        tick(px, orc, run, np.random.default_rng(0x5704 + n), 68, 10, 4, ntracks=n, blend=True, lut=lut_of(orc), order=1, wt_src=2, wt_sink=2, yvu_sink=True, pad=(4, 0, 2))


@case("tick:flat-canvas")
def _(px, orc, tune):
    """lgpu_chain_flat_yuv420p into a canvas: the bars are written by the same call"""
    from tests.test_chain_flat import run
    tick(px, orc, run, np.random.default_rng(0x5705), 36, 22, 0, ntracks=2, blend=True, lut=lut_of(orc), canvas=(40, 27, 3, 2), swap=1)


@case("tick:flat422-33-yuv420p")
def _(px, orc, tune):
    from tests.test_chain_flat422 import run, YUV422P
    tick(px, orc, run, np.random.default_rng(0x5706), YUV422P, 68, 10, 4, ntracks=33, blend=True, lut=lut_of(orc), order=1, wt_sink=2, pad=(4, 0, 2))


@case("tick:flat422-canvas")
def _(px, orc, tune):
    from tests.test_chain_flat422 import run, YUYV
    tick(px, orc, run, np.random.default_rng(0x5707), YUYV, 68, 10, 0, ntracks=2, blend=True, lut=lut_of(orc), swap=1, wt_src=1, pad=(4, 1, 3), canvas=(73, 13, 3, 1))


@case("tick:mix420-33")
def _(px, orc, tune):
    """lgpu_chain_flat_yuv420p_mix: LGPU_CHAIN_MIX_TRACKS = 32 tracks per launch"""
    from tests.test_chain_flat_mix import run_mix, layer
    tick(px, orc, run_mix, np.random.default_rng(0x5708), 68, 10, 0, ntracks=33, lut=lut_of(orc), swap=1, L1=layer(wt=1, pad=(4, 1, 3)), L2=layer(wt=1, pad=(0, 3, 1)))


@case("tick:mix420-yuv420p")
def _(px, orc, tune):
    from tests.test_chain_flat_mix import run_mix, layer
    tick(px, orc, run_mix, np.random.default_rng(0x5709), 68, 10, 4, ntracks=2, lut=lut_of(orc), order=1, L1=layer(wt=2, pad=(4, 0, 2)), L2=layer(wt=3, pad=(2, 2, 0), yvu=True),
         wt_sink=2, yvu_sink=True)


@case("tick:mix-33")
def _(px, orc, tune):
    """lgpu_chain_flat_yuv_mix, YUV422P over UYVY, 33 tracks: two launches"""
    from tests.test_chain_flat_mix422 import go, case as mcase, layer, UYVY, YUV422P
    from tests.chain_ref import distinct_amounts
    c = mcase([0x570A, 33], UYVY, YUV422P, 68, 10, 0, ntracks=33, L1=layer(wt=1, pad=(4, 0, 0)), L2=layer(wt=2, pad=(0, 3, 1)), amounts=distinct_amounts(np.random.default_rng(0x570A), 33))
    tick(px, orc, go, c, swap=1, with_lut=True)


@case("tick:mix_canvas-33")
def _(px, orc, tune):
    """lgpu_chain_flat_yuv_mix_canvas: bars and both layers, 33 tracks: two launches"""
    from tests.test_chain_flat_mix_canvas import run
    from tests.test_chain_flat_mix422 import case as mcase, layer, YUYV, YUV422P
    from tests.chain_ref import distinct_amounts
    c = mcase([0x570B, 33], YUV422P, YUYV, 6, 5, ntracks=33, L1=layer(pad=(4, 1, 3)), L2=layer(wt=1, pad=(0, 3, 1)), amounts=distinct_amounts(np.random.default_rng(0x570B), 33))
    tick(px, orc, run, c, (10, 8, 1, 2), lut=lut_of(orc), swap=1)


@case("own:repack-595-512")
def _(px, orc, tune):
    """lgpu_yuv_repack 4:1:1 -> 4:2:0 with an even height: fold chunks, walk, stream-ordered scratch (three launches)"""
    place = aa.pl()
    aa.run_repack(orc, aa.Stage(None, place), 595, 512, 40, 0)
    if px is not None:
        assert aa.run_repack(orc, StreamStage(px, place, tune), 595, 512, 40, 0) == "k_yuv411_repack"


def flat_dev(px, a):
    """a host array on the device, recorded"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    px.record(t)
    return t


def download(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@case("own:copy-fill-rows")
def _(px, orc, tune):
    """lgpu_copy, lgpu_fill, lgpu_copy_rows: what memcpy, memset and a pitched row copy give"""
    rng = aa.seeded("own", "copy")
    src, dst = rng.integers(0, 256, (9, 100), dtype=np.uint8), rng.integers(0, 256, (9, 120), dtype=np.uint8)
    want_copy = dst.copy().reshape(-1)
    want_copy[:700] = src.reshape(-1)[:700]
    want_rows = dst.copy()
    want_rows[:7, :77] = src[:7, :77]
    want_fill = dst.copy().reshape(-1)
    want_fill[:333] = 0xA7
    if px is None:
        return
    s = flat_dev(px, src)
    d = [flat_dev(px, dst) for _ in range(3)]
    px.lib.call("lgpu_copy", d[0].data_ptr(), s.data_ptr(), 700, None)
    px.lib.call("lgpu_copy_rows", d[1].data_ptr(), 120, s.data_ptr(), 100, 77, 7, None)
    px.lib.call("lgpu_fill", d[2].data_ptr(), 0xA7, 333, None)
    assert (download(d[0]).reshape(-1) == want_copy).all() and (download(d[1]) == want_rows).all() and (download(d[2]).reshape(-1) == want_fill).all()
    assert (download(s) == src).all()


@case("own:upload-small")
def _(px, orc, tune):
    """lgpu_upload of pageable memory below the staging threshold (256 KiB)"""
    src = aa.seeded("own", "upload").integers(0, 256, 5000, dtype=np.uint8)
    if px is None:
        return
    d = flat_dev(px, np.zeros(6000, np.uint8))
    px.lib.call("lgpu_upload", d.data_ptr(), src.ctypes.data, 5000, None)
    got = download(d)
    assert (got[:5000] == src).all() and not got[5000:].any()


@case("own:params_set")
def _(px, orc, tune):
    """lgpu_params_set / lgpu_params_set_n: the values travel as kernel arguments"""
    import torch
    vals = aa.seeded("own", "params").integers(-2 ** 31, 2 ** 31, 4 * 19, dtype=np.int64).astype(np.int32)       # 19 blocks: two launches of lgpu_params_set_n
    if px is None:
        return
    one, many = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4 * 19 + 4, dtype=torch.int32, device="cuda")
    px.record(one, many)
    px.lib.call("lgpu_params_set", one.data_ptr(), vals.ctypes.data, None)
    px.lib.call("lgpu_params_set_n", many.data_ptr(), vals.ctypes.data, 19, None)
    assert (download(one) == vals[:4]).all() and (download(many)[:76] == vals).all() and not download(many)[76:].any()


@case("own:letterbox_at")
def _(px, orc, tune):
    """lgpu_letterbox_at: the frame at (offs_x, offs_y) on black, as tests/test_chain_flat_mix_canvas.py's letterboxed() writes it"""
    rng = aa.seeded("own", "letterbox_at")
    w, h, nw, nh, ox, oy = 33, 5, 40, 9, 5, 3
    src = frame(rng, w, h, 4)
    before = rng.integers(0, 256, (nh + 2, align(nw * 4 + 16)), dtype=np.uint8)
    want = before.copy()
    want[:nh, :nw * 4] = np.tile(np.array([0, 0, 0, 255], np.uint8), nw)
    want[oy:oy + h, ox * 4:(ox + w) * 4] = src[:h, :w * 4]
    if px is None:
        return
    s, d = flat_dev(px, src), flat_dev(px, before)
    px.lib.call("lgpu_letterbox_at", s.data_ptr(), s.stride(0), w, h, d.data_ptr(), d.stride(0), nw, nh, 4, (ctypes.c_uint8 * 4)(0, 0, 0, 255), ox, oy, None)
    assert (download(d) == want).all()


@case("own:chain_canvas")
def _(px, orc, tune):
    """lgpu_chain_canvas: 2:1 (frame and blended bars in one launch) and 3:2 (the scaler with the chain's last stages in its store, then the bars launch), against
    tests/test_pixbuf_scale.py's composition of the oracle"""
    from tests.test_pixbuf_scale import _want_canvas
    rng = aa.seeded("own", "chain_canvas")
    lut = aa.l2s_lut(orc)
    for (sw, sh, dw, dh, nw, nh, ox, oy, swap, bf) in ((128, 16, 64, 8, 72, 12, 4, 2, 1, 77), (96, 12, 64, 8, 73, 11, 5, 2, 0, 128)):
        srcs = [frame(rng, sw, sh, 4, stride=sw * 4, alpha_mix=True) for _ in range(2)]
        l2s = [frame(rng, nw, nh, 4, stride=nw * 4, alpha_mix=True) for _ in range(2)]
        wants = [_want_canvas(orc, srcs[i], sw * 4, sw, sh, l2s[i], nw * 4, dw, dh, nw, nh, ox, oy, swap, 0x103, bf, lut) for i in range(2)]
        if px is None:
            continue
        dd = [flat_dev(px, np.full((nh, nw * 4), 0x5A, np.uint8)) for _ in range(2)]
        prm = px.chain_params(sw, sh, sw * 4, dw, dh, nw * 4, nw * 4, swap_rb=swap, interp=0x103, do_blur=0, bf=bf, lut=lut)
        px.chain_canvas(prm, px.chain_tracks([flat_dev(px, a) for a in srcs], [flat_dev(px, a) for a in l2s], dd), nw, nh, ox, oy)
        for i in range(2):
            assert (download(dd[i]) == wants[i]).all(), "chain_canvas %dx%d -> %dx%d on %dx%d track %d" % (sw, sh, dw, dh, nw, nh, i)


# ---- stateful handles: seven frames behind ONE busy period
def bz_frames(rng, w, h, n, compact):
    from tests.test_gpu_parity import bz_sequence
    return bz_sequence(rng, w, h, n, compact)


def blurzoom_sequence(px, orc, palette, mode, w, h):
    rng = aa.seeded("seq", "blurzoom", palette, mode)
    seq = bz_frames(rng, w, h, 7, compact=mode in (1, 2))
    z = orc.orc_blurzoom_new(w, h, palette)
    wants = []
    for f, a in enumerate(seq):
        want = np.full_like(a, 0x5A)
        assert orc.orc_blurzoom_process(z, P(a), a.strides[0], P(want), want.strides[0], mode, f & 3) == 0
        wants.append(want)
    orc.orc_blurzoom_free(z)
    if px is None:
        return
    srcs, dsts = [flat_dev(px, a) for a in seq], [flat_dev(px, np.full_like(a, 0x5A)) for a in seq]
    raw = px._ops

    def warm():          # the same frames through a handle of its own: the device tables and kernels are loaded, the judged handle is untouched
        g = raw.Blurzoom(w, h, palette)
        for f in range(7):
            g.process(srcs[f], dsts[f], mode, f & 3)
        px.side.synchronize()
        g.close()
    g = px.Blurzoom(w, h, palette)
    try:
        with px.batch(warm=warm):
            for f in range(7):
                g.process(srcs[f], dsts[f], mode, f & 3)
        for f in range(7):
            got = download(dsts[f])
            assert (got[:h, :w * 4] == wants[f][:h, :w * 4]).all(), "blurzoom pal=%d mode=%d frame %d of 7 behind one busy period differs from the oracle's sequence" % (palette, mode, f)
    finally:
        g.close()


@case("seq:blurzoom-mode0")
def _(px, orc, tune):
    blurzoom_sequence(px, orc, 3, 0, 70, 12)


@case("seq:blurzoom-mode1")
def _(px, orc, tune):
    """strobe: the snapshot frame inside the handle is rewritten every few frames"""
    blurzoom_sequence(px, orc, 4, 1, 64, 9)


def rgbdelay_sequence(px, orc, palette, w, h, plans, inplace=False):
    """plans: (groups, maxcache) per frame, the first one for the priming frame.  lgpu_rgbdelay_process waits for its stream on the first frame of a geometry (the ring
    restarts: stencil.hip), so frame 0 runs and is synchronised before the busy period; the seven frames after it are enqueued behind it back to back"""
    from tests import golden_util as gu
    rng = aa.seeded("seq", "rgbdelay", palette, w, h, inplace)
    s = orc.orc_rgbdelay_new()
    frames, wants, prms = [], [], []
    for groups, maxcache in plans:
        on, strength = gu.rgbdelay_params(groups)
        src = frame(rng, w, h, 3)
        want = src.copy() if inplace else np.full_like(src, 0x5A)
        a = want if inplace else src
        assert orc.orc_rgbdelay_process(s, P(a), a.strides[0], P(want), want.strides[0], w, h, palette, 1, maxcache, on.ctypes.data, strength.ctypes.data) == 0
        frames.append(src), wants.append(want), prms.append((maxcache, on, strength))
    orc.orc_rgbdelay_free(s)
    if px is None:
        return
    import torch
    srcs = [flat_dev(px, a) for a in frames]
    dsts = srcs if inplace else [flat_dev(px, np.full_like(a, 0x5A)) for a in frames]
    raw = px._ops

    def play(rd, first, last):
        for f in range(first, last):
            rd.process(srcs[f], dsts[f], w, h, palette, *prms[f], yuv_clamped=True)

    def warm():          # the whole sequence through a handle of its own
        tmp = raw.RgbDelay()
        play(tmp, 0, len(frames))
        px.side.synchronize()
        tmp.close()
    rd = px.RgbDelay()
    try:
        with torch.cuda.stream(px.side):
            play(rd._real, 0, 1)
        px.side.synchronize()
        assert (download(dsts[0]) == wants[0]).all(), "rgbdelay priming frame"
        with px.batch(warm=warm):
            play(rd, 1, len(frames))
        for f in range(1, len(frames)):
            assert (download(dsts[f]) == wants[f]).all(), "rgbdelay pal=%d frame %d behind one busy period differs from the oracle's sequence" % (palette, f)
    finally:
        rd.close()


A1 = ({0: (1, 0, 0, 1.0), 3: (0, 1, 0, 0.8), 6: (0, 0, 1, 1.0)}, 12)
A2 = ({0: (0, 1, 1, 0.9), 2: (1, 0, 0, 1.0), 6: (1, 1, 0, 0.6)}, 12)          # other switches and strengths, the same ring depth (7): no resize of the ring
FIVE = ({0: (1, 1, 1, 0.5), 1: (1, 1, 1, 0.5), 3: (1, 0, 1, 0.7), 5: (0, 1, 0, 0.4), 8: (1, 0, 0, 0.9)}, 12)       # five jobs: the table goes through pinned staging
DEEP = ({0: (1, 0, 0, 1.0), 3: (0, 1, 0, 0.8), 9: (0, 0, 1, 1.0)}, 12)        # ring depth 10


@case("seq:rgbdelay")
def _(px, orc, tune):
    """parameters change mid-sequence, ring depth constant, at most four jobs (kernel arguments): no call may wait"""
    rgbdelay_sequence(px, orc, 1, 70, 24, [A1] * 4 + [A2] * 4)


@case("seq:rgbdelay-inplace-yuv")
def _(px, orc, tune):
    rgbdelay_sequence(px, orc, 588, 72, 10, [A2] * 3 + [A1] * 5, inplace=True)


@case("seq:rgbdelay-tables")
def _(px, orc, tune):
    """five jobs per frame: every frame uploads its table through the handle's one pinned staging block, behind the `copied` event"""
    rgbdelay_sequence(px, orc, 2, 72, 10, [FIVE] * 8)


@case("seq:rgbdelay-ring")
def _(px, orc, tune):
    """the ring grows from 7 to 10 frames at the fourth judged frame"""
    rgbdelay_sequence(px, orc, 1, 70, 24, [A1] * 4 + [DEEP] * 4)


# ---- back to back: two calls with different inputs and parameters behind one busy period
def two_stages(px, orc, tune, runner, params_a, params_b, place=None):
    """one runner of tests/test_address_alignment.py twice, with different parameters (and so different inputs), into buffers of their own.  Inside the batch the entry
    points are only queued, so the runners' uploads happen before anything is enqueued; their comparisons are kept until both calls have run"""
    place = place or aa.pl()
    if px is None:
        for prm in (params_a, params_b):
            runner(orc, aa.Stage(None, place), *prm)
        return

    class Deferred(StreamStage):
        checks = None

        def check(self, name, want, rows, what):
            self.checks.append((name, want.copy(), rows, what))

    stages = [Deferred(px, place, tune) for _ in (0, 1)]
    with px.batch():
        for st, prm in zip(stages, (params_a, params_b)):
            st.checks = []
            runner(orc, st, *prm)
    for st in stages:
        assert st.checks
        for name, want, rows, what in st.checks:
            aa.Stage.check(st, name, want, rows, what + " (back to back)")


@case("b2b:swizzle-lut")
def _(px, orc, tune):
    """swizzle.hip: two LUTs"""
    two_stages(px, orc, tune, aa.run_swizzle, ("swap3", 1, 1), ("swap3postalpha", 1, 1))


@case("b2b:byte_luts")
def _(px, orc, tune):
    """effects.hip: the tables travel as kernel arguments"""
    two_stages(px, orc, tune, aa.run_byte_luts, (3,), (4,))


@case("b2b:composite")
def _(px, orc, tune):
    """stencil.hip / compositor: layer tables of two calls"""
    two_stages(px, orc, tune, aa.run_composite, (3, 0, 0), (4, 1, 1))


@case("b2b:chain_amounts")
def _(px, orc, tune):
    """pixbuf.hip, lgpu_chain_amounts: amounts, LUT and stages differ"""
    two_stages(px, orc, tune, aa.run_chain_pb, (128, 16, 64, 8, 0, 0, 1), (128, 16, 64, 8, 1, aa.OPAQUE, 1))


@case("b2b:pixbuf_scale")
def _(px, orc, tune):
    """pixbuf.hip: two geometries, each with its cached tables"""
    two_stages(px, orc, tune, aa.run_pixbuf, (4, 96, 12, 32, 4, 3, 1), (4, 64, 8, 96, 12, 3, 1))


@case("b2b:resize")
def _(px, orc, tune):
    """resize.hip: two geometries through the per-stream scratch and the table cache"""
    two_stages(px, orc, tune, aa.run_resize, (3, 136, 20, 68, 10), (3, 50, 14, 67, 20))


@case("b2b:yuv420p_to_rgb")
def _(px, orc, tune):
    """yuv.hip: with and without the LUT, two output sizes"""
    two_stages(px, orc, tune, aa.run_yuv420p, (4, 0, 1, 1), (3, 1, 0, 1))


@case("b2b:yuv_repack")
def _(px, orc, tune):
    """palette.hip: the 4:1:1 fold twice through its stream-ordered scratch, two widths"""
    two_stages(px, orc, tune, aa.run_repack, (595, 512, 40, 0), (595, 512, 72, 0))


@case("b2b:upload")
def _(px, orc, tune):
    """runtime.hip: three pageable buffers of 5 MiB (two staging chunks of 4 MiB each) -- the second upload meets both chunks in flight"""
    rng = aa.seeded("b2b", "upload")
    n = 5 << 20
    bufs = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(3)]
    if px is None:
        return
    import torch
    dsts = [torch.zeros(n + 64, dtype=torch.uint8, device="cuda") for _ in range(3)]
    px.record(dsts)
    with px.batch():
        for b, d in zip(bufs, dsts):
            px.lib.call("lgpu_upload", d.data_ptr(), b.ctypes.data, n, None)
    for i, (b, d) in enumerate(zip(bufs, dsts)):
        got = download(d)
        assert (got[:n] == b).all() and not got[n:].any(), "upload %d of three back to back" % i


@case("b2b:mix")
def _(px, orc, tune):
    """flat.hip, lgpu_chain_flat_yuv_mix: two ticks that differ in track count, formats, sink, amounts and LUT.  The tick runners upload and compare inside one call,
    so each runs twice here: once to put its frames on the device and keep the entry-point call back, then -- both kept calls back to back behind one busy period --
    its own comparison with the oracle on those very buffers"""
    from tests.test_chain_flat_mix422 import go, case as mcase, layer, UYVY, YUV422P, YUV420P
    ca = mcase([0x5B2B, 0], UYVY, YUV422P, 36, 10, 0, ntracks=3, L1=layer(wt=1, pad=(4, 0, 0)), L2=layer(wt=2, pad=(0, 3, 1)))
    cb = mcase([0x5B2B, 1], YUV420P, UYVY, 36, 10, 4, ntracks=2, L1=layer(pad=(2, 1, 1)), L2=layer(wt=1))
    ticks = [(ca, dict(swap=1, with_lut=True)), (cb, dict(order=1, wt_sink=2))]
    if px is None:
        for c, kw in ticks:
            inspect.signature(go).bind(None, orc, c, **kw)
        return
    import tests.test_chain_flat_mix422 as m

    class Resume(Exception):
        pass

    class Hold:
        """the proxy as go() sees it.  First pass: the entry point is kept back and the runner left at that point (its frames stay on the device).  Second pass: the
        uploads return the buffers of the first pass and the entry point does nothing, so that the runner compares what the back-to-back calls wrote"""

        def __init__(self):
            self.kept, self.replay = None, False

        def __getattr__(self, name):
            if name == "chain_flat_yuv_mix":
                def entry(*a, **k):
                    if not self.replay:
                        self.kept = (a, k)
                        raise Resume()
                return entry
            return getattr(px, name)
    holds, uploads = [Hold(), Hold()], [[], []]
    real_dev, real_dev_at = m.dev, m.dev_at

    def keep(i, t):
        uploads[i].append(t)
        return t
    try:
        for i, (c, kw) in enumerate(ticks):
            m.dev = lambda a, i=i: keep(i, real_dev(a))
            m.dev_at = lambda a, off, i=i: keep(i, real_dev_at(a, off))
            with pytest.raises(Resume):
                go(holds[i], orc, c, **kw)
        with px.batch():
            for h in holds:
                px.chain_flat_yuv_mix(*h.kept[0], **h.kept[1])
        for i, (c, kw) in enumerate(ticks):
            again = iter(uploads[i])
            m.dev = lambda a: next(again)
            m.dev_at = lambda a, off: next(again)
            holds[i].replay = True
            go(holds[i], orc, c, **kw)
    finally:
        m.dev, m.dev_at = real_dev, real_dev_at


# ---------------------------------------------------------------------------------------------- name -> the cases that call it
SWEPT = {
    "lgpu_upload": ["own:upload-small", "b2b:upload"],
    "lgpu_copy": ["own:copy-fill-rows"],
    "lgpu_fill": ["own:copy-fill-rows"],
    "lgpu_copy_rows": ["own:copy-fill-rows"],
    "lgpu_fill_pattern": ["grp:fill_pattern-plen3"],
    "lgpu_params_set": ["own:params_set"],
    "lgpu_params_set_n": ["own:params_set"],
    "lgpu_swizzle": ["grp:swizzle-swap3", "b2b:swizzle-lut"],
    "lgpu_swizzle_batch": ["grp:swizzle_batch-swap3"],
    "lgpu_gamma_apply": ["grp:gamma-ps4-af0-rect1"],
    "lgpu_gamma_apply_batch": ["grp:gamma_batch-ps4-af0"],
    "lgpu_alpha_premult": ["grp:premult-af0-un0"],
    "lgpu_alpha_premult_batch": ["grp:premult_batch-af0-un0"],
    "lgpu_alpha_premult_yuva": ["grp:premult_yuva-589-clamped1-un0", "grp:premult_yuva-545-clamped1-un0"],
    "lgpu_yuv420p_to_rgb": ["grp:yuv420p_to_rgb-ops4-422_0", "b2b:yuv420p_to_rgb"],
    "lgpu_yuv420p_to_rgb_batch": ["grp:yuv420p_to_rgb_batch-ops4-422_0"],
    "lgpu_yuv420p_to_rgb_lut16": ["grp:yuv420p_to_rgb_lut16"],
    "lgpu_letterbox": ["grp:letterbox-ps4"],
    "lgpu_letterbox_batch": ["grp:letterbox_batch-ps4"],
    "lgpu_letterbox_at": ["own:letterbox_at"],
    "lgpu_letterbox_bars": ["grp:letterbox_bars-ps4"],
    "lgpu_resize": ["grp:resize-ps4-136x20-68x10", "grp:resize-ps4-200x60-133x40", "grp:resize-ps3-136x20-68x10", "b2b:resize"],
    "lgpu_pixbuf_scale": ["grp:pixbuf-ch4-2to1-interp3-strips64_1", "grp:pixbuf-ch3-3to2", "b2b:pixbuf_scale"],
    "lgpu_pixbuf_scale_batch": ["grp:pixbuf_batch-ch4-2to1-interp3"],
    "lgpu_gauss5": ["grp:gauss5-ps4-40x12", "grp:gauss5-ps3-40x12"],
    "lgpu_gauss5_colorkey": ["grp:gauss5_colorkey-ps4"],
    "lgpu_blend_chroma": ["grp:chroma-ps4-0"],
    "lgpu_blend_luma": ["grp:luma-ps4-3"],
    "lgpu_blend_multi": ["grp:multi-ps3-5"],
    "lgpu_colorkey": ["grp:colorkey-ps3-0"],
    "lgpu_colorkey_batch": ["grp:colorkey_batch"],
    "lgpu_rgb_to_yuv": ["grp:rgb_to_yuv-order0-alpha1-fmt4"],
    "lgpu_rgb_to_yuv_batch": ["grp:rgb_to_yuv_batch-fmt4"],
    "lgpu_rgb_to_yuv_lut16": ["grp:rgb_to_yuv_lut16-order0-alpha0-fmt2"],
    "lgpu_yuv_to_rgb": ["grp:yuv_to_rgb-fmt2-ia0-order2-oa1"],
    "lgpu_yuv_to_rgb_batch": ["grp:yuv_to_rgb_batch-fmt2"],
    "lgpu_yuv411_to_rgb": ["grp:yuv411_to_rgb-order0-alpha0"],
    "lgpu_rgb_to_yuv411": ["grp:rgb_to_yuv411-order0-alpha0"],
    "lgpu_yuv_switch_clamping": ["grp:clamp_switch-512"],
    "lgpu_yuv_repack": ["grp:repack-512-564-w40", "grp:repack-565-595-w40", "own:repack-595-512", "b2b:yuv_repack"],
    "lgpu_softlight": ["grp:softlight-544-w40", "grp:softlight-512-w40"],
    "lgpu_fx_batch": ["grp:fx_batch-softlight-544", "grp:fx_batch-transition-ps4", "grp:fx_batch-gauss5_colorkey-ps4", "grp:fx_batch-chroma-ps4",
                      "grp:fx_batch-yuv411_to_rgb-order0-alpha0"],
    "lgpu_edge": ["grp:edge-pal2-mode2", "grp:edge-pal2-mode2-inplace", "grp:edge-pal4-mode2", "grp:edge-pal4-mode2-inplace"],
    "lgpu_blurzoom_process": ["seq:blurzoom-mode0", "seq:blurzoom-mode1"],
    "lgpu_rgbdelay_process": ["seq:rgbdelay", "seq:rgbdelay-inplace-yuv", "seq:rgbdelay-tables", "seq:rgbdelay-ring"],
    "lgpu_transition": ["grp:transition-kind1-ps4"],
    "lgpu_byte_luts": ["grp:byte_luts-ps3", "b2b:byte_luts"],
    "lgpu_deinterlace": ["grp:deinterlace-pal3-w21", "grp:deinterlace-pal3-w21-inplace"],
    "lgpu_triple_split": ["grp:triple_split-rows1"],
    "lgpu_slide_over": ["grp:slide_over-dir1-ps4"],
    "lgpu_dissolve": ["grp:dissolve-ps4"],
    "lgpu_mirror": ["grp:mirror-mode2-ps4", "grp:mirror-mode0-ps3-inplace"],
    "lgpu_mirror_batch": ["grp:mirror_batch-ps4"],
    "lgpu_composite": ["grp:composite-ps4-bgr1-revz0", "b2b:composite"],
    "lgpu_chain": ["grp:chain-136x20-68x10-blur1", "grp:chain-200x60-133x40-blur0", "grp:chain_pixbuf-128x16-64x8-blur0-flag0-amounts0",
                   "grp:chain_pixbuf-128x16-64x8-blur1-flag200-amounts0"],
    "lgpu_chain_canvas": ["own:chain_canvas"],
    "lgpu_chain_amounts": ["grp:chain_pixbuf-128x16-64x8-blur0-flag0-amounts1", "grp:chain_pixbuf-96x12-64x8-blur1-flag0", "grp:chain_canvas-blur1-noblend0", "b2b:chain_amounts"],
    "lgpu_chain_yuv420p": ["grp:chain_yuv420p-tight1-canvas1", "tick:chain_yuv420p-canvas"],
    "lgpu_chain_to_yuv": ["grp:chain_sink-fmt4-yuvsrc0", "tick:chain_to_yuv-33"],
    "lgpu_chain_yuv420p_to_yuv": ["grp:chain_sink-fmt4-yuvsrc1", "tick:transcode-33-yuv420p", "tick:transcode-64-yuv420p"],
    "lgpu_chain_flat_yuv420p": ["tick:flat-canvas"],
    "lgpu_chain_flat_yuv420p_to_yuv": ["tick:flat-33-yuv420p", "tick:flat-64-yuv420p"],
    "lgpu_chain_flat_yuv420p_mix": ["tick:mix420-33", "tick:mix420-yuv420p"],
    "lgpu_chain_flat_yuv422": ["tick:flat422-33-yuv420p", "tick:flat422-canvas"],
    "lgpu_chain_flat_yuv_mix": ["tick:mix-33", "b2b:mix"],
    "lgpu_chain_flat_yuv_mix_canvas": ["tick:mix_canvas-33"],
}
NAMES_OF = collections.defaultdict(set)          # case -> the entry points it must reach
for _name, _ids in SWEPT.items():
    for _cid in _ids:
        NAMES_OF[_cid].add(_name)


# ---------------------------------------------------------------------------------------------- CPU tests
def test_every_stream_taking_prototype_is_swept_or_exempt():
    """a new entry point with a `void *stream` cannot be added without a stream case or a stated reason"""
    assert len(STREAM_NAMES) == len(set(STREAM_NAMES)) >= 80
    assert not set(SWEPT) & set(EXEMPT)
    missing = [n for n in STREAM_NAMES if n not in SWEPT and n not in EXEMPT]
    assert not missing, "include/lives_gpu.h has stream-taking prototypes that tests/test_stream_order.py neither sweeps nor exempts: %s" % missing
    gone = sorted((set(SWEPT) | set(EXEMPT)) - set(STREAM_NAMES))
    assert not gone, "SWEPT / EXEMPT name prototypes the header no longer has (or that take no stream): %s" % gone
    for name, ids in SWEPT.items():
        assert ids and all(cid in CASES for cid in ids), "%s: SWEPT names a case that does not exist: %s" % (name, [c for c in ids if c not in CASES])
    assert all(reason for reason in EXEMPT.values())
    for cid, waits in EXPECTED_WAITS.items():
        assert cid in CASES and all(len(w) == 3 and all(w) for w in waits.values()), cid
    assert len(EXPECTED_WAITS) <= 4, "EXPECTED_WAITS must stay short"


def test_the_header_parser():
    text = """int lgpu_a(int x, void *stream);   /* int lgpu_commented(void *stream); */
    int lgpu_b(const uint8_t black_pixel[4],
               void *stream);
    int lgpu_c(void *streams);  int lgpu_d(void *stream, void *event);  // int lgpu_e(void *stream);
    void *lgpu_f(size_t bytes);"""
    assert so.stream_entry_points(text) == ["lgpu_a", "lgpu_b", "lgpu_d"]


def test_the_proxy_records_tensors_in_every_nesting():
    """the recording half of the harness, with CPU tensors and a stub module: lists of planes per frame (fx_batch), tuples of (tensor or None, ...) (composite), the
    track builders, keyword arguments, dicts, a stateful handle's process(), and the same view handed over twice counted once"""
    import types
    import torch
    stub = types.ModuleType("stub_ops")
    seen = []

    def entry(*a, **k):
        seen.append((a, k))

    def chain_tracks(srcs, layer2s, dsts):
        return ("tracks", len(srcs))

    def chain_params(sw, param_block=None):
        return ("params", sw)

    class Blurzoom:
        def __init__(self, w):
            self.w = w

        def process(self, src, dst, mode=0):
            seen.append(("bz", mode))
    for f in (entry, chain_tracks, chain_params):
        f.__module__ = stub.__name__
        setattr(stub, f.__name__, f)
    stub.Blurzoom, stub.CONSTANT = Blurzoom, 7
    t = [torch.zeros(4, dtype=torch.uint8) + i for i in range(12)]
    rec = so.Recorder()
    rec.add([[t[0], t[1]], [t[2]]], ((t[3], 1, 2), (None, 3, 4)), {"a": t[4], "b": [t[5], {"c": (t[6],)}]}, 5, "x", None, t[0])
    assert [id(x) for x in rec.tensors] == [id(x) for x in t[:7]]
    rec.add(t[0][1:], t[0][:])                               # another view is another entry; the same range is not
    assert len(rec.tensors) == 8

    class Px(so.StreamProxy):                                # recording only: the steps that need a device are replaced by the plain call
        def _judge(self, calls, warm):
            return [fn(*a, **k) for _, fn, a, k in calls]
    px = Px(stub, side=None)
    assert px.CONSTANT == 7
    assert px.chain_tracks([t[0], t[1]], None, [t[2]]) == ("tracks", 2) and px.chain_params(3, param_block=t[3]) == ("params", 3)
    px.entry([[t[4]], [t[5]]], k=(t[6], None))
    g = px.Blurzoom(9)
    g.process(t[7], dst=t[8], mode=2)
    assert g.w == 9 and seen[-1] == ("bz", 2)
    px.record(t[9])
    assert [id(x) for x in px.rec.tensors] == [id(x) for x in t[:10]]
    with px.batch():
        assert px.entry(t[10]) is None and len(seen) == 2    # queued, not run
        px.entry(t[11])
    assert len(seen) == 4 and len(px.rec.tensors) == 12
    c = so.complement(torch.tensor([0.5, -2.0]))
    assert c.dtype == torch.float32 and (so.complement(c) == torch.tensor([0.5, -2.0])).all()
    assert so.is_host_helper("chain_yuv_mix_tracks") and so.is_host_helper("resize_plan") and not so.is_host_helper("chain") and not so.is_host_helper("yuv_repack")


def test_every_case_is_accepted_without_a_gpu(orc):
    """the dry pass: every sweep case builds its inputs and runs the oracle (the cases of tests/test_address_alignment.py and this module's own), or binds its
    arguments to the runner it calls (the tick forms' runners upload for themselves)"""
    for cid, fn in CASES.items():
        try:
            fn(None, orc, None)
        except Exception as e:
            raise AssertionError("%s: %s: %s" % (cid, type(e).__name__, e)) from e


def test_the_multi_launch_shapes_are_in_the_table():
    """the entry points that split a tick into several launches, cross-checked against the constants of the dispatch code"""
    def const(path, pattern):
        import re
        with open(os.path.join(ROOT, path)) as f:
            return int(re.search(pattern, f.read()).group(1))
    assert const("lives_amd/csrc/flat.hip", r"constexpr int kFlatPlanarTracks = (\d+);") == 32          # tick:flat-33 / -64: two launches
    assert const("include/lives_gpu.h", r"#define LGPU_CHAIN_TRANSCODE_TRACKS (\d+)") == 32              # tick:transcode-33 / -64
    assert const("include/lives_gpu.h", r"#define LGPU_CHAIN_MIX_TRACKS (\d+)") == 32                    # tick:mix420-33, tick:mix-33, tick:mix_canvas-33
    for cid in ("tick:flat-33-yuv420p", "tick:flat-64-yuv420p", "tick:transcode-33-yuv420p", "tick:transcode-64-yuv420p", "tick:mix420-33", "tick:mix-33", "tick:mix_canvas-33",
                "tick:flat-canvas", "tick:chain_yuv420p-canvas", "grp:chain-136x20-68x10-blur1", "grp:chain-200x60-133x40-blur0", "grp:chain_pixbuf-96x12-64x8-blur1-flag0", "own:chain_canvas",
                "grp:resize-ps3-136x20-68x10", "grp:gauss5-ps4-40x12", "grp:edge-pal2-mode2", "grp:edge-pal4-mode2", "grp:edge-pal2-mode2-inplace", "grp:edge-pal4-mode2-inplace",
                "own:repack-595-512", "grp:premult_yuva-589-clamped1-un0", "grp:softlight-544-w40"):
        assert cid in CASES, cid


# ---------------------------------------------------------------------------------------------- teeth
def side_stream():
    return so.side_stream()


class Fakes:
    """what the teeth tests call through the proxy: torch ops only"""

    def __init__(self):
        import types
        self.mod = types.ModuleType("fake_ops")

    def add(self, fn):
        fn.__module__ = self.mod.__name__
        setattr(self.mod, fn.__name__, fn)
        return self.mod


def teeth_buffers():
    import torch
    g = torch.Generator(device="cpu").manual_seed(7)
    src = torch.randint(0, 256, (64, 256), dtype=torch.uint8, generator=g).cuda()
    return src, torch.zeros_like(src), src.cpu().numpy().copy()


@G
def test_teeth_a_call_on_the_default_stream_is_a_byte_mismatch(gpu):
    import torch
    side = side_stream()

    def stray(src, dst):
        with torch.cuda.stream(torch.cuda.default_stream()):
            dst.copy_(src)
    px = so.StreamProxy(Fakes().add(stray), side)
    src, dst, want = teeth_buffers()
    px.stray(src, dst)
    assert (download(src) == want).all()
    assert (download(dst) != want).any(), "the harness did not notice a copy made on the default stream"


@G
def test_teeth_a_stray_first_stage_is_a_byte_mismatch(gpu):
    """only the scratch stage strayed: src -> scratch on the default stream, scratch -> dst on the side stream.  It reads the complemented source"""
    import torch
    side = side_stream()
    scratch = torch.zeros((64, 256), dtype=torch.uint8, device="cuda")

    def two_stage(src, dst):
        with torch.cuda.stream(torch.cuda.default_stream()):
            scratch.copy_(src)
        dst.copy_(scratch)
    px = so.StreamProxy(Fakes().add(two_stage), side)
    src, dst, want = teeth_buffers()
    px.two_stage(src, dst)
    assert (download(dst) != want).any(), "the harness did not notice a first stage on the default stream"


@G
def test_teeth_a_wait_trips_the_event(gpu):
    side = side_stream()

    def waits(src, dst):
        dst.copy_(src)
        side.synchronize()
    px = so.StreamProxy(Fakes().add(waits), side)
    src, dst, want = teeth_buffers()
    px.waits(src, dst)
    assert (download(dst) == want).all()
    assert px.calls[0].waited
    with pytest.raises(AssertionError, match="waits waited for its stream.*warm-up .* ms, call .* ms on the host, busy period"):
        px.finish()
    listed = so.StreamProxy(Fakes().add(waits), side, expect_wait=lambda name, index: name == "waits")
    listed.waits(src, dst)
    listed.finish()


@G
def test_teeth_a_well_behaved_call_passes_both(gpu):
    side = side_stream()

    def good(src, dst):
        dst.copy_(src)
    px = so.StreamProxy(Fakes().add(good), side)
    src, dst, want = teeth_buffers()
    px.good(src, dst)
    assert (download(dst) == want).all() and (download(src) == want).all()
    (c,) = px.finish()
    assert not c.waited and c.busy_real >= 0.5 * c.busy_ms
    listed = so.StreamProxy(Fakes().add(good), side, expect_wait=lambda name, index: True)        # listed as a call that waits: it must
    listed.good(src, dst)
    with pytest.raises(AssertionError, match="is listed as a call that waits, and did not"):
        listed.finish()
    with px.batch():                                                                             # two calls behind one busy period
        px.good(src, dst)
        px.good(dst, src)
    assert len(px.finish()) == 3 and (download(src) == want).all()


# ---------------------------------------------------------------------------------------------- the sweep
# one test per runner of tests/test_address_alignment.py (all of its groups) and per kind of this module's own cases: the suite's list of tests stays short
BUNDLES = collections.OrderedDict()
for _cid in CASES:
    _key = _cid.split(":")[0] if not _cid.startswith("grp:") else [g[1].__name__[4:] for g in aa.GROUPS if "grp:" + g[0] == _cid][0]
    BUNDLES.setdefault(_key, []).append(_cid)


def test_every_case_is_in_one_bundle():
    assert sorted(c for ids in BUNDLES.values() for c in ids) == sorted(CASES) and len(BUNDLES) < 40


def run_case(gpu, orc, tune, monkeypatch, cid):
    """one case through the proxy: the bytes of the oracle after synchronising the side stream only, every judged call returned while the stream was busy (or waited,
    where EXPECTED_WAITS says so), and the entry points SWEPT attributes to this case were really called.  Returns the judged calls"""
    from lives_amd import lib
    reached, real_call = set(), lib.call

    def spy(name, *args):
        reached.add(name)
        return real_call(name, *args)
    with monkeypatch.context() as mp:
        mp.setattr(lib, "call", spy)
        px = so.StreamProxy(gpu, side_stream(), expect_wait=expect_wait(cid), stream_names=STREAM_NAMES)
        CASES[cid](px, orc, tune)
    calls = px.finish()
    assert calls, "%s made no judged call" % cid
    assert NAMES_OF[cid] <= reached, "%s is listed in SWEPT for %s and did not call it" % (cid, sorted(NAMES_OF[cid] - reached))
    return calls


@G
@pytest.mark.parametrize("bundle", list(BUNDLES))
def test_on_a_busy_side_stream(gpu, orc, tune, monkeypatch, bundle):
    """every case of one bundle, each through a proxy of its own (run_case); a failing case does not hide the ones after it"""
    failures, calls = [], []
    for cid in BUNDLES[bundle]:
        try:
            calls += run_case(gpu, orc, tune, monkeypatch, cid)
        except AssertionError as e:
            failures.append("%s: %s" % (cid, e))
    judged = [c for c in calls if c.judged]
    print("stream-order: %s: %d cases, %d judged calls, %d waited as listed, largest warm-up %.3f ms, largest busy period %.1f ms (%s)" % (
        bundle, len(BUNDLES[bundle]), len(judged), sum(c.waited for c in judged), max([c.t_warm for c in calls] or [0]), max([c.busy_ms for c in calls] or [0]),
        "%.0f %s per ms" % (so.BUSY.per_ms, so.BUSY.kind)))
    assert not failures, "%d of %d cases failed:\n%s" % (len(failures), len(BUNDLES[bundle]), "\n".join(failures))


# ---------------------------------------------------------------------------------------------- cold start
def cold_expectations(orc):
    """inputs and the oracle's results of the child's calls, by name"""
    rng = aa.seeded("cold")
    out = {}
    w, h = 40, 6
    # a 4:2:0 sink conversion (ensure_cavgc)
    src = frame(rng, w, h, 4)
    want, _ = po.k4_out_planes(0, w, h, 4, 0)
    wp, ws = po.planes_args(want)
    assert orc.orc_rgb_to_yuv(P(src), src.strides[0], w, h, 0, 1, ctypes.addressof(wp), ctypes.addressof(ws), 4, 0, 0) == 0
    out.update(sink420_src=src, sink420_y=want[0], sink420_u=want[1], sink420_v=want[2])
    # an opaque 2:1 chain on the gdk-pixbuf arithmetic (pb_opaque_check) and the same chain to a YUV sink (get_sink_tables)
    sw, sh, dw, dh = 128, 16, 64, 8
    csrc, l2 = frame(rng, sw, sh, 4), frame(rng, dw, dh, 4, alpha_mix=True)
    csrc[:, 3::4] = 255
    lut = aa.l2s_lut(orc)
    from tests.chain_ref import oracle_chain_rgba
    cw = oracle_chain_rgba(orc, csrc, sw, sh, dw, dh, 3, 1, l2, 77, lut)
    out.update(chain_src=csrc, chain_l2=l2, chain_lut=lut, opaque_chain=cw)
    rgba = oracle_chain_rgba(orc, csrc, sw, sh, dw, dh, 3, 0, l2, 77, lut)
    sink, _ = po.k4_out_planes(0, dw, dh, 2, 0)
    sp, ss = po.planes_args(sink)
    assert orc.orc_rgb_to_yuv(P(rgba), rgba.strides[0], dw, dh, 0, 1, ctypes.addressof(sp), ctypes.addressof(ss), 2, 0, 1) == 0
    out.update(chain_to_yuv=sink[0])
    # a pixbuf scale and a polyphase resize off 2:1 (table caches)
    a = frame(rng, 96, 12, 4, alpha_mix=True)
    pw = np.zeros((8, 64 * 4), np.uint8)
    assert orc.orc_pixbuf_scale(P(a), a.strides[0], 96, 12, P(pw), 64 * 4, 64, 8, 4, 3) == 0
    rw = np.zeros((40, align(133 * 4)), np.uint8)
    b = frame(rng, 200, 60, 4)
    assert orc.orc_resize(P(b), b.strides[0], 200, 60, P(rw), rw.strides[0], 133, 40, 4, 3) == 0
    out.update(pixbuf_src=a, pixbuf_scale=pw, resize_src=b, resize=rw)
    # edge (the per-stream state is created and zeroed by the first call), an in-place deinterlace (the snapshot grows), clamped premultiply (its tables)
    e = frame(rng, 40, 12, 4)
    ew = np.full_like(e, 0x5A)
    orc.orc_edge(P(e), e.strides[0], P(ew), ew.strides[0], 40, 12, 3, 2, P(np.zeros(40 * 12, np.int16)), 0)
    d = frame(rng, 21, 8, 4)
    d[1:8:2] = (d[1:8:2] >> 2) + 160
    dwant = d.copy()
    assert orc.orc_deinterlace(P(dwant), dwant.strides[0], P(dwant), dwant.strides[0], 21, 8, 3) == 0
    y = frame(rng, 40, 6, 4)
    yw = y.copy()
    yp, ys = (ctypes.c_void_p * 4)(yw.ctypes.data, None, None, None), (ctypes.c_int * 4)(yw.strides[0], 0, 0, 0)
    orc.orc_alpha_premult_yuva(yp, ys, 40, 6, 589, 1, 0)
    out.update(edge_src=e, edge=ew[:, :160], deint_src=d, deinterlace_inplace=dwant, premult_src=y, premult_yuva=yw)
    return out


CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from lives_amd import lib, ops
from tests.stream_order import BUSY, side_stream
z = np.load(sys.argv[2])
lib.load()
ops.init(0)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
src420, csrc, l2, pa, rb, es, dd, yy = (up(z[k]) for k in ("sink420_src", "chain_src", "chain_l2", "pixbuf_src", "resize_src", "edge_src", "deint_src", "premult_src"))
planes = [torch.full(z[k].shape, 0x5A, dtype=torch.uint8, device="cuda") for k in ("sink420_y", "sink420_u", "sink420_v")]
new = lambda k: torch.full(z[k].shape, 0x5A, dtype=torch.uint8, device="cuda")
o_chain, o_sink, o_pb, o_rs, o_edge = new("opaque_chain"), new("chain_to_yuv"), new("pixbuf_scale"), new("resize"), torch.full(z["edge_src"].shape, 0x5A, dtype=torch.uint8, device="cuda")
lut = z["chain_lut"]
side = side_stream()
torch.cuda.synchronize()
with torch.cuda.stream(side):
    BUSY.enqueue(50.0)
    # the first call ever of each lazily initialising path, on the busy stream
    ops.rgb_to_yuv(src420, planes, 40, 6, 0, 1, 4, 0, 0)
    prm = ops.chain_params(128, 16, csrc.stride(0), 64, 8, l2.stride(0), 256, swap_rb=1, interp=3 | 0x100 | 0x200, do_blur=0, bf=77, lut=lut)      # LGPU_INTERP_OPAQUE
    ops.chain(prm, ops.chain_tracks([csrc], [l2], [o_chain]))
    prm2 = ops.chain_params(128, 16, csrc.stride(0), 64, 8, l2.stride(0), 0, swap_rb=0, interp=3 | 0x100, do_blur=0, bf=0, lut=lut)
    ops.chain_to_yuv(prm2, ops.chain_sink(2, [o_sink.stride(0)], which_tables=1, in_order=0), ops.chain_sink_tracks([csrc], [l2], [[o_sink]]), [77])
    ops.pixbuf_scale(pa, o_pb, 96, 12, 64, 8, channels=4, interp=3)
    ops.resize(rb, o_rs, 200, 60, 133, 40, psize=4, interp=3)
    ops.edge(es, o_edge, 40, 12, 3, 2)
    ops.deinterlace(dd, dd, 21, 8, 3)
    ops.alpha_premult_yuva([yy], 40, 6, 589, 1, 0)
side.synchronize()
got = {"sink420_y": planes[0], "sink420_u": planes[1], "sink420_v": planes[2], "opaque_chain": o_chain, "chain_to_yuv": o_sink, "pixbuf_scale": o_pb, "resize": o_rs,
       "edge": o_edge[:, :160], "deinterlace_inplace": dd, "premult_yuva": yy}
bad = []
for k, t in got.items():
    g, w = t.cpu().numpy(), z[k]
    cols = {"resize": 133 * 4, "deinterlace_inplace": 21 * 4, "premult_yuva": 160}.get(k, w.shape[1])
    if not (g[:, :cols] == w[:, :cols]).all():
        bad.append("%s: %d bytes differ" % (k, int((g[:, :cols] != w[:, :cols]).sum())))
print("cold start:", bad or "every first call equals the oracle")
sys.exit(1 if bad else 0)
"""


def test_the_cold_start_expectations_build(orc):
    z = cold_expectations(orc)
    assert all(isinstance(v, np.ndarray) for v in z.values()) and {"opaque_chain", "chain_to_yuv", "edge", "resize"} <= set(z)


@G
def test_first_ever_calls_on_a_busy_side_stream(gpu, orc, tmp_path):
    """one fresh process: the library is initialised, a side stream made busy, and each lazily initialising path called for the first time ever on it -- the
    chroma-average table of a 4:2:0 sink, the opaque check and the sink tables of the 2:1 chain, the scalers' table caches, lgpu_edge's per-stream state, the snapshot of
    an in-place deinterlace, the clamped premultiply tables.  A table built or zeroed on another stream than the one its first reader runs on shows as a mismatch"""
    path = str(tmp_path / "cold.npz")
    np.savez(path, **cold_expectations(orc))
    script = tmp_path / "cold_child.py"
    script.write_text(CHILD)
    try:
        r = subprocess.run([sys.executable, str(script), ROOT, path], timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired as e:
        pytest.exit("the cold-start child hung and was ended: nothing further is started on this device\n%s" % (e.stdout or "")[-2000:], returncode=3)
    if r.returncode in (124, 134, 137, 139, -6, -9, -11, -15):
        pytest.exit("the cold-start child ended with status %d: nothing further is started on this device\n%s" % (r.returncode, r.stdout[-2000:]), returncode=3)
    assert r.returncode == 0, "the cold-start child failed (status %d):\n%s" % (r.returncode, r.stdout[-3000:])
