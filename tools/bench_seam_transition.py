#!/usr/bin/env python3
"""tools/bench_seam_transition.py -- a tick of transitions between two DECODED clips through the layer seam: 16 pinned tracks of 1920x1080, both layers of every track
decoder frames (YUV420P / YUV422P / UYVY), the reference's calls per track -- convert_layer_palette of layer 2, convert_layer_palette of layer 1, livesgpu_fx.so's
"chroma blend", gamma_convert_layer [, convert_layer_palette_full to UYVY] -- and ONE lives_gpu_layers_flush per tick.  One more case letterboxes 1440x1080 frames of
both layers into 1920x1080.

What is compared (lives_gpu_set_pending_layer2, include/lives_gpu_layer.h), with lives_gpu_set_flat_yuv(1) throughout:
  mode 0 -- today: every second layer runs alone, on the calling thread, when its blend is recorded (16 one-frame launches), then one launch for the readers;
  mode 3 -- the second layers stay pending and run as ONE group ahead of their readers: two launches per tick;
  mode 2 -- the second layers are folded into their readers' launch (lgpu_chain_flat_yuv_mix[_canvas]): one launch per tick.
A host clock around `--ticks` ticks that end in one device synchronise; every tick has fresh pinned layers (made, uploaded and synchronised before the clock starts) drawn
from `--sets` different frames, so no tick reads what the one before left in the caches.  The modes alternate inside one process for `--rounds` interleaved rounds; per mode
the best round and the spread (max - min) over the rounds are printed, in microseconds per tick, host calls included.  A library without the setter (the parent commit's
build: --lib-dir) runs today's path alone, which is the baseline mode 0 is printed beside.  One JSON line per case.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RGBA32, YUV420P, YUV422P, UYVY = 3, 512, 522, 564
NAMES = {YUV420P: "YUV420P", YUV422P: "YUV422P", UYVY: "UYVY"}
PW, PH = 1920, 1080
# (layer 2 over layer 1, the README's order), sink palette or None, frame size (letterboxed into PW x PH when smaller)
CASES = [(YUV420P, YUV420P, None, (PW, PH)), (UYVY, YUV420P, None, (PW, PH)), (YUV420P, UYVY, None, (PW, PH)), (YUV422P, YUV422P, None, (PW, PH)),
         (YUV420P, YUV420P, UYVY, (PW, PH)), (UYVY, YUV420P, UYVY, (PW, PH)), (YUV420P, UYVY, UYVY, (PW, PH)), (YUV422P, YUV422P, UYVY, (PW, PH)),
         (YUV420P, YUV420P, None, (1440, PH))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=6, help="ticks inside one clocked region")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sets", type=int, default=3, help="different frames per layer the ticks rotate over")
    ap.add_argument("--lib-dir", default=None, help="a directory with another build's liblivesgpu.so and livesgpu_fx.so (the parent commit's: the baseline)")
    ap.add_argument("--cases", default=None, help="comma-separated case numbers (default: all)")
    args = ap.parse_args()
    if args.lib_dir:
        os.environ["LGPU_SO"] = os.path.join(os.path.abspath(args.lib_dir), "liblivesgpu.so")
    import numpy as np
    import torch
    from lives_amd import lib
    from oracle import pyoracle as po
    if not po.have_ref():
        print("skipped: oracle/_ref (the reference libweed the host side needs) is not built")
        return 0
    from tests import weedhost as wh
    L = lib.load()
    wh.bind(L)
    L.lives_gpu_layers_flush.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
    L.lives_gpu_deferred_stats_n.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    L.lives_gpu_deferred_stats_n.restype = None
    has_setter = hasattr(L, "lives_gpu_set_pending_layer2")
    modes = [0, 3, 2] if has_setter else [None]
    assert L.lives_gpu_set_flat_yuv(1) in (0, 1)
    H = po.RefHost()
    fx = os.path.join(os.path.abspath(args.lib_dir) if args.lib_dir else os.path.join(ROOT, "lives_amd"), "livesgpu_fx.so")
    libc = ctypes.CDLL("libc.so.6")
    libc.free.argtypes = [ctypes.c_void_p]
    n = args.tracks
    rng = np.random.default_rng(0x7A51)

    def frames(pal, w, h):
        if pal == UYVY:
            return [rng.integers(0, 256, (h, w * 2), dtype=np.uint8)]
        ch = h // 2 if pal == YUV420P else h
        return [rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, w // 2), dtype=np.uint8), rng.integers(0, 256, (ch, w // 2), dtype=np.uint8)]

    def layer(pal, w, h, planes):
        return wh.new_layer(pal, w // 2 if pal == UYVY else w, h, planes, gamma=1, clamping=0, subspace=1)

    def stats():
        a = (ctypes.c_ulonglong * 19)()
        L.lives_gpu_deferred_stats_n(a, 19)
        return list(a)

    def pointers(lay):
        """the layer's plane pointers and rowstrides without copying the planes (tests/weedhost.py's planes_of copies them)"""
        W = wh.weed()
        k = ctypes.c_int()
        pd = W.weed_get_voidptr_array_counted(lay, b"pixel_data", ctypes.byref(k))
        rs = W.weed_get_int_array_counted(lay, b"rowstrides", ctypes.byref(ctypes.c_int()))
        return [pd[i] for i in range(k.value)], [rs[i] for i in range(k.value)]

    def view(lay):
        """a numpy view ON the layer's host plane (the address a channel of weed_apply_instance would carry)"""
        ptrs, rs = pointers(lay)
        hh = wh.geti(lay, "height")
        return np.frombuffer((ctypes.c_uint8 * (rs[0] * hh)).from_address(ptrs[0]), np.uint8).reshape(hh, rs[0])

    def one_round(p2, p1, sink, size, mode):
        """`--ticks` ticks under one clock: us per tick, and the counter deltas of the last tick"""
        w, h = size
        canvas = (PW, PH) if size != (PW, PH) else None
        if mode is not None:
            L.lives_gpu_set_pending_layer2(mode)
        ticks = []
        for t in range(args.ticks):
            lays = [layer(p1, w, h, src1[(t + i) % args.sets]) for i in range(n)]
            l2l = [layer(p2, w, h, src2[(t + i) % args.sets]) for i in range(n)]
            for a in lays + l2l:
                assert L.lives_gpu_layer_pin(a) == 0          # the decoder frames' uploads: before the clock starts
            ticks.append((lays, l2l))
        torch.cuda.synchronize()
        d = None
        t0 = time.perf_counter()
        for lays, l2l in ticks:
            s0 = stats()
            for i in range(n):
                for a in (l2l[i], lays[i]):
                    assert L.lives_gpu_convert_layer_palette(a, RGBA32, 0) == 1
                    if canvas:
                        assert L.lives_gpu_letterbox_layer(a, canvas[0], canvas[1], w, h, 3, RGBA32, 0) == 1
                v, v2 = view(lays[i]), view(l2l[i])
                H.run(fx, "chroma blend", RGBA32, PW, PH, [v, v2], v, [po.p_int((40 + 13 * i) & 0xFF)])
                assert L.lives_gpu_gamma_convert_layer(2, lays[i]) == 1
                if sink:
                    assert L.lives_gpu_convert_layer_palette_full(lays[i], sink, 0, 0, 1, 2) == 1
            assert L.lives_gpu_layers_flush((ctypes.c_void_p * n)(*lays), n) == 0
            d = [b - a for a, b in zip(s0, stats())]
        torch.cuda.synchronize()                              # every stream of the device: the seam enqueues on the calling thread's own
        us = (time.perf_counter() - t0) * 1e6 / args.ticks
        for lays, l2l in ticks:
            for a in lays + l2l:
                ptrs = pointers(a)[0]
                assert L.lives_gpu_layer_forget(a) == 0
                libc.free(ptrs[0])                            # every layer ends as one plane (RGBA or UYVY) of its own allocation
        return us, d

    which = [int(x) for x in args.cases.split(",")] if args.cases else range(len(CASES))
    print("build: %s" % ("this tree" if not args.lib_dir else args.lib_dir + (" (no lives_gpu_set_pending_layer2: today's path)" if not has_setter else "")))
    print("| layer 2 over layer 1 | to | frames | mode | best us per tick | spread over %d rounds | launches per tick [1] / pre [7] / mix [16] / layer 2 first [18] |" % args.rounds)
    print("|---|---|---|---|---|---|---|")
    for c in which:
        p2, p1, sink, size = CASES[c]
        src1 = [frames(p1, *size) for _ in range(args.sets)]
        src2 = [frames(p2, *size) for _ in range(args.sets)]
        one_round(p2, p1, sink, size, modes[0])                  # warm: tables, pool buffers, the plugin
        res = {m: [] for m in modes}
        last = {}
        for _ in range(args.rounds):
            for m in modes:
                us, d = one_round(p2, p1, sink, size, m)
                res[m].append(us)
                last[m] = d
        out = {"tool": "bench_seam_transition", "case": c, "layer2": NAMES[p2], "layer1": NAMES[p1], "sink": NAMES.get(sink, "RGBA"), "frames": "%dx%d" % size, "tracks": n,
               "ticks": args.ticks, "rounds": args.rounds, "parent_build": not has_setter}
        for m in modes:
            best, spread, d = min(res[m]), max(res[m]) - min(res[m]), last[m]
            name = "today" if m is None else str(m)
            print("| %s over %s | %s | %dx%d%s | %s | %.1f | %.1f | %d / %d / %d / %d |" % (NAMES[p2], NAMES[p1], NAMES.get(sink, "RGBA"), size[0], size[1],
                  " in %dx%d" % (PW, PH) if size != (PW, PH) else "", name, best, spread, d[1], d[7], d[16], d[18]), flush=True)
            out["mode_%s" % name] = {"best_us": round(best, 1), "spread_us": round(spread, 1), "rounds_us": [round(x, 1) for x in res[m]], "counters": d}
        print(json.dumps(out), flush=True)
    if has_setter:
        L.lives_gpu_set_pending_layer2(0)
    L.lives_gpu_set_flat_yuv(0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
