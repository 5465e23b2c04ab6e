"""Every stream-taking entry point captured into a HIP graph and replayed: the bytes of the oracle after the SECOND replay (the first and only one for handles).

DESIGN.md section 2 promises that steady-state launches neither allocate nor synchronise and capture into HIP graphs; tools/bench_ops.py publishes graph-replay figures and
silently falls back to the eager one where a capture fails.  tests/graph_replay.py:GraphProxy stands where the cases of tests/test_stream_order.py expect their proxy
(its docstring has the seven steps) and turns that table -- every stream-taking prototype of the header, every case compared with the oracle bit for bit -- into a
capture-and-replay sweep.

  inventory   NOT_CAPTURED: the cases whose entry point allocates, waits or keeps host state once warm, each with the source line that does it and what a host calls
              instead.  They are not attempted on the GPU.  Every other case is swept; every entry point but lgpu_upload keeps a captured case
  proxy       the recording and host-scramble halves, with CPU tensors and a stub module
  teeth       the harness catches a stage outside the captured stream, a read of caller host memory at replay and device state that only the host resets, with torch ops
              only; the allocator probe flags the staged gdk-pixbuf chain and not the fused one
  sweep       every bundle of test_stream_order.BUNDLES, and this module's own cases (MORE), by itself, two bundles to a test (CHAPTERS), every case with a proxy of its own
  handle      lgpu_blurzoom_process in modes 0 and 3 keeps its whole state on the device: ONE captured process() call replays frame after frame
"""
import collections
import os
import time

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import graph_replay as gr
from tests import test_address_alignment as aa
from tests import test_stream_order as tso
from tests.test_stream_order import test_every_case_is_accepted_without_a_gpu          # noqa: F401 -- the dry pass: every case builds its inputs and its oracle result with px=None
from tests.test_wide_frames import squeeze

G = pytest.mark.gpu
P = po.P
ROOT = tso.ROOT
CASES, BUNDLES, SWEPT, NAMES_OF = tso.CASES, tso.BUNDLES, tso.SWEPT, tso.NAMES_OF
CAP = 20

STAGED = ("pixbuf.hip: if ((rc = lgpu_malloc_ordered(&sa, per * group, st))) return rc;",
          "a STAGED chain (include/lives_gpu.h lists the forms at lgpu_chain; here: the gdk-pixbuf chain with the gaussian off the exact aligned 2:1 ratio, onto a canvas "
          "or without layer 2) runs stage by stage through scratch frames from the stream-ordered pool, taken and given back by every call: make this call between graph "
          "launches on the same stream; lgpu_chain without LGPU_INTERP_PIXBUF and the aligned 2:1 pixbuf chain capture with the gaussian")
REPACK = ("palette.hip: if ((rc = lgpu_malloc_ordered(&tab, (size_t)2 * nch * 256, st))) return rc;",
          "YUV411 -> 4:2:0 with an even height takes its fold table from the stream-ordered pool per call: call it between graph launches on the same stream "
          "(every other pair of lgpu_yuv_repack is one launch and captures)")
# case -> (entry point, file: the source line that allocates / waits / keeps host state, what a host does instead)
NOT_CAPTURED = {
    "own:upload-small": ("lgpu_upload", "runtime.hip: LGPU_HIP(hipMemcpyAsync(dst_d, src_h, bytes, hipMemcpyHostToDevice, st));",
                         "a copy node keeps the caller's host pointer and reads it at every replay: upload before the graph (order the streams with lgpu_event_record / "
                         "lgpu_stream_wait_event), or send small blocks as kernel arguments with lgpu_params_set"),
    "b2b:upload": ("lgpu_upload", "runtime.hip: if (t_stage.busy[k]) LGPU_HIP(hipEventSynchronize(t_stage.ev[k]));",
                   "pageable uploads are copied into pinned staging chunks on the host at call time and wait for the chunk's last DMA: upload outside the graph"),
    "seq:rgbdelay-tables": ("lgpu_rgbdelay_process", "stencil.hip: if (s->in_flight) { LGPU_HIP(hipEventSynchronize(s->copied)); s->in_flight = false; }",
                            "more than four jobs travel through the handle's one pinned staging table, filled at call time behind an event wait: call it between graph launches"),
    "seq:rgbdelay-ring": ("lgpu_rgbdelay_process", "stencil.hip: for (int i = s->tcache; i > maxneeded; i--) { (void)hipFree(s->cache[i - 1]); s->cache[i - 1] = nullptr; }",
                          "a change of the ring's depth synchronises the stream and resizes the ring with hipMalloc / hipFree: change the depth outside a capture"),
    "own:repack-595-512": ("lgpu_yuv_repack",) + REPACK,
    "b2b:yuv_repack": ("lgpu_yuv_repack",) + REPACK,
    "grp:chain_pixbuf-96x12-64x8-blur1-flag0": ("lgpu_chain_amounts",) + STAGED,
    "grp:chain_pixbuf-96x12-64x8-blur1-flag400": ("lgpu_chain_amounts",) + STAGED,
    "grp:chain_canvas-blur1-noblend0": ("lgpu_chain_amounts",) + STAGED,
    # 2:1, but the class whose frames miss k_pb_half's alignment goes stage by stage as well
    "grp:chain_pixbuf-128x16-64x8-blur1-flag0-amounts1": ("lgpu_chain_amounts",) + STAGED,
    "grp:chain_pixbuf-128x16-64x8-blur1-flag200-amounts0": ("lgpu_chain",) + STAGED,
}
# the entry points that cannot be captured at all (their header comments say so): no case of theirs needs to stay
NEVER = {"lgpu_upload"}


# ---------------------------------------------------------------------------------------------- this module's own cases (the bundle "more")
MORE = collections.OrderedDict()          # id -> (fn(px, orc, tune), the entry points it must reach inside a capture)


def more(cid, *names):
    def reg(fn):
        assert cid not in CASES and cid not in MORE
        MORE[cid] = (fn, set(names))
        return fn
    return reg


@more("own:chain-half-blur1", "lgpu_chain")
def _(px, orc, tune):
    """lgpu_chain (one amount for all tracks, from bf) on the gdk-pixbuf arithmetic WITH the gaussian at the exact aligned 2:1 case: one launch of k_pb_half, the form
    the documents name as the capturable gaussian chain.  The groups that reach it are listed in NOT_CAPTURED for their misaligned class"""
    place = aa.pl()
    assert aa.run_chain_pb(orc, aa.Stage(None, place), 128, 16, 64, 8, 1, 0, 0) == "k_pb_half chain"
    if px is not None:
        assert aa.run_chain_pb(orc, tso.StreamStage(px, place, tune), 128, 16, 64, 8, 1, 0, 0) == "k_pb_half chain"


@more("own:params_set-host", "lgpu_params_set", "lgpu_params_set_n")
def _(px, orc, tune):
    """own:params_set again with the caller's value block named to the proxy (the runtime's calls take raw addresses, which carry no array): it is complemented while the
    graph replays, so values read from host memory at replay -- instead of travelling as kernel arguments -- show"""
    vals = aa.seeded("more", "params").integers(-2 ** 31, 2 ** 31, 4 * 19, dtype=np.int64).astype(np.int32)       # 19 blocks: two launches of lgpu_params_set_n
    keep = vals.copy()
    if px is None:
        return
    import torch
    one, many = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4 * 19 + 4, dtype=torch.int32, device="cuda")
    px.record(one, many)
    px.record_host(vals)
    px.lib.call("lgpu_params_set", one.data_ptr(), vals.ctypes.data, None)
    px.lib.call("lgpu_params_set_n", many.data_ptr(), vals.ctypes.data, 19, None)
    assert (vals == keep).all(), "the proxy left the caller's block scrambled"
    assert (tso.download(one) == keep[:4]).all() and (tso.download(many)[:76] == keep).all() and not tso.download(many)[76:].any()


ALL_CASES = collections.OrderedDict(list(CASES.items()) + [(cid, fn) for cid, (fn, _) in MORE.items()])
ALL_BUNDLES = collections.OrderedDict(list(BUNDLES.items()) + [("more", list(MORE))])


def names_of(cid):
    return MORE[cid][1] if cid in MORE else NAMES_OF[cid]


def swept_cases(bundle):
    return [cid for cid in ALL_BUNDLES[bundle] if cid not in NOT_CAPTURED]


# the sweep's tests: two bundles each, in the table's order; every bundle still runs, prints and is timed by itself
CHAPTERS = [list(ALL_BUNDLES)[i:i + 2] for i in range(0, len(ALL_BUNDLES), 2)]


# ---------------------------------------------------------------------------------------------- CPU tests
def test_every_case_is_swept_or_listed():
    assert len(CASES) >= 300 and set(NOT_CAPTURED) <= set(CASES), sorted(set(NOT_CAPTURED) - set(CASES))
    assert len(NOT_CAPTURED) <= CAP, "%d cases are listed as not capturable: more than %d is a finding about the library, not a longer list" % (len(NOT_CAPTURED), CAP)
    assert sorted(c for b in ALL_BUNDLES for c in swept_cases(b)) == sorted((set(CASES) | set(MORE)) - set(NOT_CAPTURED))
    assert [b for chapter in CHAPTERS for b in chapter] == list(BUNDLES) + ["more"] and all(names <= set(tso.STREAM_NAMES) for _, names in MORE.values())
    for cid, entry in NOT_CAPTURED.items():
        assert len(entry) == 3 and all(entry), cid
        assert entry[0] in NAMES_OF[cid] or entry[0] in tso.STREAM_NAMES, (cid, entry[0])
    for cid, waits in tso.EXPECTED_WAITS.items():
        assert cid in NOT_CAPTURED, "%s waits for its stream once warm (EXPECTED_WAITS) and is not in NOT_CAPTURED" % cid
        for name, _, _ in waits.values():
            assert NOT_CAPTURED[cid][0].replace("lgpu_", "").replace("_process", "") in name.lower().replace("lgpu_", "").replace(".process", ""), (cid, name)


def test_this_modules_own_cases_are_accepted_without_a_gpu(orc):
    for cid, (fn, _) in MORE.items():
        fn(None, orc, None)


def test_every_listed_line_is_in_the_sources():
    """a listed reason names the line that allocates, waits or keeps host state: when that line goes, the entry goes (or follows it)"""
    texts = {}
    for cid, (_, where, _) in NOT_CAPTURED.items():
        fname, line = where.split(": ", 1)
        if fname not in texts:
            with open(os.path.join(ROOT, "lives_amd", "csrc", fname)) as f:
                texts[fname] = squeeze(f.read())
        assert squeeze(line) in texts[fname], "%s: lives_amd/csrc/%s no longer has the line `%s`" % (cid, fname, line)


def test_every_entry_point_keeps_a_captured_case():
    for name, ids in SWEPT.items():
        if name in NEVER:
            assert all(cid in NOT_CAPTURED for cid in ids), "%s is said never to capture, and %s are swept" % (name, [c for c in ids if c not in NOT_CAPTURED])
            continue
        assert [cid for cid in ids if cid not in NOT_CAPTURED], "%s has lost its last captured case: add one at a shape that takes its non-allocating form" % name
    with open(os.path.join(ROOT, "include", "lives_gpu.h")) as f:
        header = f.read()
    for name in sorted({e[0] for e in NOT_CAPTURED.values()} | {"lgpu_blurzoom_process"}):
        at = header.index("\nint %s(" % name)
        assert "capture" in header[header.rindex("/*", 0, at):at], "include/lives_gpu.h: the comment above %s does not say what a stream capture can expect of it" % name


def test_the_scramble_finds_restores_and_spares():
    """numpy arrays are found in every nesting, complemented once however often they are handed over, read-only ones left alone, and everything is as it was after
    an exception"""
    a, b, c, d = np.arange(12, dtype=np.uint8), np.linspace(0, 1, 5), np.arange(6, dtype=np.int32).reshape(2, 3), np.arange(4, dtype=np.uint8)
    ro = np.arange(5, dtype=np.uint8)
    ro.flags.writeable = False
    strided = np.arange(20, dtype=np.int16)[::2]
    zero = np.array(7, dtype=np.int32)
    keep = [x.copy() for x in (a, b, c, d, ro, strided, zero)]
    args = ((a, [b, {"k": (c,)}], 3, "x", None, a[2:5], zero), {"kw": [strided, ro], "again": a, "d": {"e": [d]}})
    found = gr.arrays_in(args, [])
    assert [id(x) for x in found[:3]] == [id(a), id(b), id(c)] and len(found) == 9
    s = gr.Scramble(args)
    assert [id(x) for x in s.arrays] == [id(a), id(b), id(c), id(zero), id(strided), id(d)]          # a's view and a again: once; the read-only one: never
    with pytest.raises(ZeroDivisionError):
        with s:
            assert (a == 255 - keep[0]).all() and (c == ~keep[2]).all() and (d == 255 - keep[3]).all() and (strided == ~keep[5]).all() and zero == ~keep[6]
            assert b.view(np.uint64)[1] == ~keep[1].view(np.uint64)[1] and (ro == keep[4]).all()
            1 / 0
    for x, k in zip((a, b, c, d, ro, strided, zero), keep):
        assert (x == k).all()
    assert (np.arange(20, dtype=np.int16)[1::2] == np.arange(1, 20, 2)).all()


def test_the_proxy_records_and_queues_like_the_stream_proxy():
    """the recording half with CPU tensors and a stub module: what reaches _judge is what StreamProxy would have judged -- single calls, a batch as one list with its
    warm callable, a handle's process() under its kind's name, lib.call rerouted for a stream-taking name"""
    import types
    import torch
    stub, seen, judged = types.ModuleType("stub_ops"), [], []

    def entry(*a, **k):
        seen.append((a, k))
        return len(seen)

    def chain_tracks(srcs, layer2s, dsts):
        return ("tracks", len(srcs))

    def stream_ptr():
        return "STREAM"

    class Blurzoom:
        def __init__(self, w):
            self.w = w

        def process(self, src, dst, mode=0):
            seen.append(("bz", mode))

    class Lib:
        @staticmethod
        def call(name, *args):
            seen.append((name, args))
    for f in (entry, chain_tracks, stream_ptr):
        f.__module__ = stub.__name__
        setattr(stub, f.__name__, f)
    stub.Blurzoom, stub.lib = Blurzoom, Lib

    class Px(gr.GraphProxy):                                 # the steps that need a device are replaced by the plain calls
        def _judge(self, calls, warm):
            judged.append(([c[0] for c in calls], warm))
            return [fn(*a, **k) for _, fn, a, k in calls]
    t = [torch.zeros(4, dtype=torch.uint8) + i for i in range(8)]
    px = Px(stub, side=None, stream_names=["lgpu_fill"], arm=None)
    assert px.chain_tracks([t[0]], None, [t[1]]) == ("tracks", 1) and not judged
    assert px.entry([t[2]], k=(t[3], np.zeros(3))) == 1 and judged[-1][0] == ["entry"]
    g = px.Blurzoom(9)
    g.process(t[4], dst=t[5], mode=2)
    assert g.w == 9 and judged[-1][0] == ["Blurzoom.process"] and gr.is_stateful("Blurzoom.process") and gr.is_stateful("RgbDelay.process") and not gr.is_stateful("entry")
    px.lib.call("lgpu_fill", 1, 2, None)
    assert seen[-1] == ("lgpu_fill", (1, 2, "STREAM")) and judged[-1][0] == ["lgpu_fill"]
    px.lib.call("lgpu_other", 1, None)
    assert seen[-1] == ("lgpu_other", (1, None)) and len(judged) == 3
    marker = lambda: None
    with px.batch(warm=marker):
        assert px.entry(t[6]) is None and g.process(t[7], t[7]) is None and len(judged) == 3
    assert judged[-1] == (["entry", "Blurzoom.process"], marker)
    px.record(t[0])
    assert [id(x) for x in px.rec.tensors] == [id(x) for x in t]
    block = np.arange(5)
    px.record_host([block], 3)
    assert [id(x) for x in px.hosts] == [id(block)] and [id(x) for x in gr.Scramble([(1,)], px.hosts).arrays] == [id(block)]
    assert px.finish() == [] and px.graphs == 0
    px.problems.append("x")
    with pytest.raises(AssertionError):
        px.finish()


# ---------------------------------------------------------------------------------------------- teeth
def fake_proxy(fn, **kw):
    return gr.GraphProxy(tso.Fakes().add(fn), tso.side_stream(), **kw)


@G
def test_teeth_a_stage_outside_the_captured_stream_ran_during_the_capture(gpu):
    import torch
    other = torch.cuda.Stream()

    def stray(src, dst):
        with torch.cuda.stream(other):
            dst[:32].copy_(src[:32])
        dst[32:].copy_(src[32:])
    px = fake_proxy(stray)
    src, dst, want = tso.teeth_buffers()
    px.stray(src, dst)
    assert px.graphs == 1
    with pytest.raises(AssertionError, match="stray: 1 of 2 recorded tensors changed during the capture"):
        px.finish()


@G
def test_teeth_a_read_of_caller_host_memory_at_replay_meets_the_scramble(gpu):
    import ctypes
    import torch
    from lives_amd import lib
    src, dst, want = tso.teeth_buffers()
    L = lib.load()
    block = L.lgpu_pinned_calloc(want.size)                    # page-locked memory that torch's own host allocator knows nothing of: it records no event of its own in the capture
    assert block
    try:
        host = np.ctypeslib.as_array(ctypes.cast(block, ctypes.POINTER(ctypes.c_uint8)), shape=(want.size,)).reshape(want.shape)
        host[...] = want
        pinned = torch.from_numpy(host)

        def late_reader(table, dst):
            dst.copy_(pinned, non_blocking=True)
        px = fake_proxy(late_reader)
        px.late_reader(host, dst)
        px.finish()                                            # nothing ran during the capture, nothing else to report
        assert (host == want).all(), "the proxy left the caller's array scrambled"
        assert (tso.download(dst) == 255 - want).all(), "the harness did not notice a graph that reads caller host memory at replay"
        del pinned, host
    finally:
        torch.cuda.synchronize()
        L.lgpu_pinned_free(block)


def counting_fake():
    """a call that expects its device counter to be zero: the host resets it before every call (on a stream of the fake's own, outside any graph, and waits for that
    where waiting is allowed), the captured work checks and increments it"""
    import torch
    counter, own = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.cuda.Stream()
    torch.cuda.synchronize()

    def counted(src, dst):
        with torch.cuda.stream(own):
            counter.zero_()
        if not torch.cuda.is_current_stream_capturing():
            own.synchronize()
        dst.copy_(src)
        dst.mul_(counter.eq(0).to(torch.uint8))
        counter.add_(1)
    return counted


@G
def test_teeth_device_state_the_host_resets_shows_in_the_second_replay(gpu):
    src, dst, want = tso.teeth_buffers()
    once = fake_proxy(counting_fake(), replays=1)
    once.counted(src, dst)
    once.finish()
    assert (tso.download(dst) == want).all(), "the first replay of the counting fake should still be right"
    twice = fake_proxy(counting_fake())
    twice.counted(src, dst)
    twice.finish()
    assert not tso.download(dst).any(), "the harness did not notice device state that only the host resets"


@G
def test_teeth_a_well_behaved_call_passes_all_three(gpu):
    def good(src, dst):
        dst.copy_(src)
    px = fake_proxy(good)
    src, dst, want = tso.teeth_buffers()
    table = np.arange(7)
    px.good(src, dst)
    with px.batch():                                           # two calls in ONE graph
        px.good(src, dst)
        px.good(dst, src)
    assert px.finish() == ["good"] * 3 and px.graphs == 2 and not px.eager
    assert (tso.download(dst) == want).all() and (tso.download(src) == want).all() and (table == np.arange(7)).all()


@G
def test_the_allocator_probe_flags_the_staged_chain_and_not_the_fused_one(gpu, orc, tune):
    """lgpu_chain_amounts at 96x12 -> 64x8 with the gaussian takes its scratch frames from the stream-ordered pool in every call; at 128x16 -> 64x8 without it the chain is
    one launch.  Probe only: nothing is captured here"""
    staged = gr.GraphProxy(gpu, tso.side_stream(), stream_names=tso.STREAM_NAMES, capture=False)
    aa.run_chain_pb(orc, tso.StreamStage(staged, aa.pl(), tune), 96, 12, 64, 8, 1, 0, 1)          # (its comparison with the oracle runs on the eager result)
    assert staged.flagged == ["chain_amounts"] and staged.graphs == 0
    with pytest.raises(AssertionError, match=r"chain_amounts reaches lgpu_malloc / lgpu_malloc_ordered once warm .*\(-5\).*injected"):
        staged.finish()
    fused = gr.GraphProxy(gpu, tso.side_stream(), stream_names=tso.STREAM_NAMES, capture=False)
    aa.run_chain_pb(orc, tso.StreamStage(fused, aa.pl(), tune), 128, 16, 64, 8, 0, 0, 1)
    assert not fused.flagged and fused.eager == ["chain_amounts"]
    fused.finish()
    # two more staged forms of include/lives_gpu.h's list that no case of the table takes: lgpu_chain_canvas without LGPU_INTERP_PIXBUF, and the gdk-pixbuf chain with
    # the NEAREST filter (no scaler kernel takes the chain's last stages there) -- neither has the gaussian
    from tests.util import frame
    rng, lut = aa.seeded("graph", "probe"), aa.l2s_lut(orc)
    for entry, interp, (sw, sh, dw, dh), canvas in (("chain_canvas", 3, (128, 16, 64, 8), (72, 12, 4, 2)), ("chain", 0 | aa.PIXBUF, (96, 12, 64, 8), None)):
        px = gr.GraphProxy(gpu, tso.side_stream(), stream_names=tso.STREAM_NAMES, capture=False)
        cw, ch = canvas[:2] if canvas else (dw, dh)
        src, l2 = tso.flat_dev(px, frame(rng, sw, sh, 4, stride=sw * 4, alpha_mix=True)), tso.flat_dev(px, frame(rng, cw, ch, 4, stride=cw * 4, alpha_mix=True))
        dst = tso.flat_dev(px, np.full((ch, cw * 4), 0x5A, np.uint8))
        prm = px.chain_params(sw, sh, sw * 4, dw, dh, cw * 4, cw * 4, swap_rb=1, interp=interp, do_blur=0, bf=77, lut=lut)
        trk = px.chain_tracks([src], [l2], [dst])
        if canvas:
            px.chain_canvas(prm, trk, *canvas)
        else:
            px.chain(prm, trk)
        assert px.flagged == [entry], "%s interp=%#x: %s" % (entry, interp, px.flagged)


# ---------------------------------------------------------------------------------------------- the sweep
def run_case(gpu, orc, tune, monkeypatch, cid, gate):
    """one case through a GraphProxy of its own: the case's comparison with the oracle judges the last replay; the entry points SWEPT attributes to the case were
    reached INSIDE a capture.  Returns the proxy"""
    import torch
    from lives_amd import lib
    inside, real_call = set(), lib.call

    def spy(name, *args):
        if torch.cuda.is_current_stream_capturing():
            inside.add(name)
        return real_call(name, *args)
    with monkeypatch.context() as mp:
        mp.setattr(lib, "call", spy)
        px = gr.GraphProxy(gpu, tso.side_stream(), stream_names=tso.STREAM_NAMES, gate=gate)
        ALL_CASES[cid](px, orc, tune)
    assert px.finish(), "%s captured no call" % cid
    assert names_of(cid) <= inside, "%s is listed for %s and did not call it inside a capture" % (cid, sorted(names_of(cid) - inside))
    return px


def sweep_bundle(gpu, orc, tune, monkeypatch, bundle, gate):
    """every case of one bundle that is not in NOT_CAPTURED; a failing case -- whatever it raises -- does not hide the ones after it, except a capture that raised: no
    further capture is made behind `gate` then.  Prints the bundle's line and returns its failures"""
    failures, ncalls, ngraphs, t0, ids = [], 0, 0, time.perf_counter(), swept_cases(bundle)
    for n, cid in enumerate(ids):
        if gate.failed:
            failures.append("the capture of %s raised: %d cases were not attempted (%s)" % (gate.failed, len(ids) - n, ", ".join(ids[n:])))
            break
        try:
            px = run_case(gpu, orc, tune, monkeypatch, cid, gate)
            ncalls, ngraphs = ncalls + len(px.captured), ngraphs + px.graphs
        except Exception as e:
            failures.append("%s: %s: %s" % (cid, type(e).__name__, e))
    print("graph-replay: %s: %d cases (%d listed as not capturable), %d captured calls in %d graphs, %.2f s" % (
        bundle, len(ids), len(ALL_BUNDLES[bundle]) - len(ids), ncalls, ngraphs, time.perf_counter() - t0))
    return ["%s: %s" % (bundle, f) for f in failures]


@G
@pytest.mark.parametrize("chapter", CHAPTERS, ids="+".join)
def test_captured_and_replayed(gpu, orc, tune, monkeypatch, chapter):
    """two bundles, one after the other, each as sweep_bundle() runs it, behind ONE gate: after a capture that raised, this test makes no further capture -- the cases
    it did not attempt are named in its failure.  (A bundle to a test would be the stream-order suite's layout; two keep the suite's list of tests shorter.)"""
    gate = gr.Gate()
    failures = [f for bundle in chapter for f in sweep_bundle(gpu, orc, tune, monkeypatch, bundle, gate)]
    assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures))


# ---------------------------------------------------------------------------------------------- blurzoom as a replayable handle
@G
def test_blurzoom_is_a_replayable_handle(gpu, orc):
    """modes 0 and 3 never touch the handle's host state (snap_time moves in the strobe modes only): after two eager frames ONE captured process() on fixed buffers
    is replayed for each of the next four frames and gives the oracle's sequence"""
    for palette, mode in ((3, 0), (4, 3)):
        blurzoom_replays(gpu, orc, palette, mode)


def blurzoom_replays(gpu, orc, palette, mode):
    import torch
    w, h, pattern, n = 70, 12, 1, 6
    rng = aa.seeded("graph", "blurzoom", palette, mode)
    seq = tso.bz_frames(rng, w, h, n, compact=False)
    z, wants = orc.orc_blurzoom_new(w, h, palette), []
    for a in seq:
        want = np.full_like(a, 0x5A)
        assert orc.orc_blurzoom_process(z, P(a), a.strides[0], P(want), want.strides[0], mode, pattern) == 0
        wants.append(want)
    orc.orc_blurzoom_free(z)
    frames = [torch.from_numpy(a).cuda() for a in seq]
    src, dst, side = torch.empty_like(frames[0]), torch.empty_like(frames[0]), tso.side_stream()
    torch.cuda.synchronize()
    bz = gpu.Blurzoom(w, h, palette)

    def feed(f, run):
        with torch.cuda.stream(side):
            src.copy_(frames[f], non_blocking=True)
            dst.fill_(0x5A)
            run()
        gr.device_is_alive("blurzoom frame %d" % f, side)
        assert (tso.download(dst)[:h, :w * 4] == wants[f][:h, :w * 4]).all(), "blurzoom pal=%d mode=%d frame %d (%s) differs from the oracle's sequence" % (
            palette, mode, f, "eager" if f < 2 else "replay %d of one captured call" % (f - 1))
    try:
        for f in (0, 1):
            feed(f, lambda: bz.process(src, dst, mode, pattern))
        g, _ = gr.capture(side, lambda: bz.process(src, dst, mode, pattern), "Blurzoom.process")
        try:
            for f in range(2, n):
                feed(f, g.replay)
        finally:
            del g
    finally:
        bz.close()
