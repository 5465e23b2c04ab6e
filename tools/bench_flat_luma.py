#!/usr/bin/env python3
"""tools/bench_flat_luma.py -- a luma overlay between two decoded clips in one launch (lgpu_chain_flat_yuv_luma, include/lives_gpu_luma.h): 16 x 1920x1080 tracks with
the gamma LUT, <layer 2> over <layer 1> each YUV420P, YUV422P or UYVY, to RGBA and to UYVY.

Two contents, on both layers alike: `noise` (every sample random: every wave is mixed at any threshold between the ends) and `structured` (columns of 128 pixels -- one
wave of the kernel -- in turn a constant dark luma, a constant bright luma and noise, chroma 128 under the constant ones: at threshold 64 a third of the waves shows only
the keyed layer and skips the other one).

Timed, by the protocol of tools/bench_flat_select.py (events on the launch stream around back-to-back launches ending in a synchronise, rotated over `--sets` buffer
sets so that a pass does not sit in the 256 MiB Infinity Cache, all forms alternated in `--rounds` rounds in the same process, the round-to-round spread reported):
  luma -- the one launch: types 1 to 4 at threshold 64 on either content, and type 1 at threshold 0 on noise;
  (a) staged -- the launches that DEFINE the bytes, in their batch forms: both conversions (lgpu_yuv420p_to_rgb_batch / lgpu_yuv_to_rgb_batch), lgpu_fx_batch
      LGPU_FX_BLEND_LUMA in place, lgpu_gamma_apply_batch [, lgpu_rgb_to_yuv_batch];
  (b) mix -- lgpu_chain_flat_yuv_mix on the same pair: the crossfade, which converts both layers everywhere;
  (c) single -- against threshold 0 only: layer 1's single-layer flat form with LGPU_INTERP_NOBLEND.
Checks first that luma and staged give the same bytes.  No ratio is fixed in advance: the figures ship as measured, and each comparison says whether the one launch is
ahead by more than the spread of the other form's rounds.  One JSON line per pair and format.  Reads nothing outside the tree."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1920, 1080
FMT = {"rgba": 0, "yuv420p": 4, "uyvy": 2, "yuyv": 3, "yuv422p": 5}
THRESHOLD, DARK, BRIGHT, BLOCK = 64, 40, 200, 128
CONTENTS = ("structured", "noise")
CASES = [("type %d %s" % (t, c), t, c, THRESHOLD) for t in (1, 2, 3, 4) for c in CONTENTS]
END = ("type 1 @0", 1, "noise", 0)


def dims(fmt):
    return [(W * 4, H)] if fmt == 0 else [(W * 2, H)] if fmt in (2, 3) else [(W, H), (W // 2, H // 2), (W // 2, H // 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds of each form")
    ap.add_argument("--sets", type=int, default=4, help="buffer sets rotated between launches (cold buffers)")
    ap.add_argument("--formats", default="rgba,uyvy")
    ap.add_argument("--pairs", default="yuv420p/yuv420p,uyvy/yuv420p", help="<layer 2>/<layer 1>, comma separated")
    args = ap.parse_args()
    import numpy as np
    import torch
    from lives_amd import lib, ops
    from oracle import pyoracle as po
    ops.init(0)
    n, S = args.tracks, args.sets
    g = torch.Generator(device="cuda")
    g.manual_seed(0x10A)
    lut = np.zeros(256, np.uint8)
    po.oracle().orc_gamma_lut8(1.0, po.GAMMA_SRGB, po.GAMMA_LINEAR, 1.4, po.P(lut))

    def rnd(r, b):
        return [torch.randint(0, 256, (r, b), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]

    def structure(f, planes):
        """every third column of 128 pixels dark, the next bright, the next left as drawn"""
        for b in range(W // BLOCK):
            if b % 3 == 2:
                continue
            v = (DARK, BRIGHT)[b % 3]
            for t in range(n):
                if f in (2, 3):
                    m = planes[0][t].view(H, W // 2, 4)[:, b * BLOCK // 2:(b + 1) * BLOCK // 2]
                    yi, ci = ((1, 3), (0, 2)) if f == 2 else ((0, 2), (1, 3))
                    for j in yi:
                        m[:, :, j] = v
                    for j in ci:
                        m[:, :, j] = 128
                else:
                    planes[0][t][:, b * BLOCK:(b + 1) * BLOCK] = v
                    for k in (1, 2):
                        planes[k][t][:, b * BLOCK // 2:(b + 1) * BLOCK // 2] = 128

    def clip(f, content):
        """the planes of n tracks (None: the format has no such plane), their strides and chroma plane bytes"""
        if f in (2, 3):
            out = [rnd(H, W * 2), None, None], (W * 2,), 0
        else:
            ch = H // 2 if f == 4 else H
            out = [rnd(H, W), rnd(ch, W // 2), rnd(ch, W // 2)], (W, W // 2, W // 2), ch * (W // 2)
        if content == "structured":
            structure(f, out[0])
        return out

    ca = [torch.zeros((H, W * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]       # the staged form's converted layers; layer 1's is blended in place
    cb = [torch.zeros((H, W * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    prm = ops.chain_params(W, H, W * 4, W, H, W * 4, W * 4, swap_rb=0, interp=0x100, bf=0, lut=lut)
    prm_single = ops.chain_params(W, H, W * 4, W, H, W * 4, W * 4, swap_rb=0, interp=0x100 | 0x400, bf=0, lut=lut)
    ok = True
    for pair in args.pairs.split(","):
        n2, n1 = pair.split("/")
        f2, f1 = FMT[n2], FMT[n1]
        l1 = {c: [clip(f1, c) for _ in range(S)] for c in CONTENTS}
        l2 = {c: [clip(f2, c) for _ in range(S)] for c in CONTENTS}
        (_, st1, csz1), (_, st2, csz2) = l1["noise"][0], l2["noise"][0]
        s1 = ops.yuv_layer_source(f1, st1, csz1, csz1, out_order=0, which_tables=0, pb_quality=2)
        s2 = ops.yuv_layer_source(f2, st2, csz2, csz2, out_order=0, which_tables=0, pb_quality=2)
        old1 = ops.yuv_source(st1, csz1, csz1, out_order=0, which_tables=0, pb_quality=2) if f1 == 4 else ops.yuv422_source(f1, st1, csz1, csz1, out_order=0, which_tables=0, pb_quality=2)
        for name in args.formats.split(","):
            fmt = FMT[name]
            dd = dims(fmt)
            new = lambda: [[[torch.zeros((r, b), dtype=torch.uint8, device="cuda") for (b, r) in dd] for _ in range(n)] for _ in range(S)]
            out_f, out_t = new(), new()
            sink = ops.chain_sink(fmt, [b for (b, _) in dd], which_tables=0, in_order=0) if fmt else None
            f_trk = {c: [ops.chain_yuv_mix_tracks(l1[c][s][0][0], l1[c][s][0][1], l1[c][s][0][2], l2[c][s][0][0], l2[c][s][0][1], l2[c][s][0][2], out_f[s]) for s in range(S)] for c in CONTENTS}
            A = l1["noise"]
            if f1 == 4 and fmt == 0:
                o_trk = [ops.chain_yuv_tracks(A[s][0][0], A[s][0][1], A[s][0][2], None, [o[0] for o in out_f[s]]) for s in range(S)]
            else:
                o_trk = [ops.chain_yuv_sink_tracks(A[s][0][0], A[s][0][1], A[s][0][2], None, out_f[s]) for s in range(S)]

            def luma(type_, content, thr):
                return lambda i: ops.chain_flat_yuv_luma(prm, s1, s2, f_trk[content][i % S], type_, [thr] * n, sink=sink)

            def convert(f, L, s, dst):
                if f in (2, 3):
                    ops.yuv_to_rgb_batch([[x] for x in L[s][0][0]], dst, W, H, f, 0, 0, 1, 0)
                else:
                    ops.yuv420p_to_rgb_batch(list(zip(L[s][0][0], L[s][0][1], L[s][0][2], dst)), W, H, 4, 0, int(f == 5), 0, 2)

            def staged(type_, content, thr):
                def run(i):
                    s = i % S
                    target = [o[0] for o in out_t[s]] if fmt == 0 else ca
                    convert(f2, l2[content], s, cb)
                    convert(f1, l1[content], s, target)
                    ops.fx_batch(ops.FX_BLEND_LUMA, [[x] for x in target], [[x] for x in target], W, H, ins1=[[x] for x in cb], ip=(type_, 4, 0, 0), dp=(float(thr), 0.))
                    tp = (ctypes.c_void_p * n)(*[t.data_ptr() for t in target])
                    lib.call("lgpu_gamma_apply_batch", tp, W * 4, 0, 0, W, H, 4, 0, ops.lut_ptr(lut)[0], n, ops.stream_ptr())
                    if fmt:
                        ops.rgb_to_yuv_batch(ca, out_t[s], W, H, 0, 1, fmt, 0, 0)
                return run

            def mix(i):
                ops.chain_flat_yuv_mix(prm, s1, s2, f_trk["noise"][i % S], [128] * n, sink=sink)

            def single(i):
                if f1 != 4:
                    ops.chain_flat_yuv422(prm_single, old1, o_trk[i % S], None, sink=sink)
                elif fmt == 0:
                    ops.chain_flat_yuv420p(prm_single, old1, o_trk[i % S], None)
                else:
                    ops.chain_flat_yuv420p_to_yuv(prm_single, old1, sink, o_trk[i % S], None)

            same = True
            for label, type_, content, thr in CASES + [END]:          # the same bytes first
                for i in range(S):
                    luma(type_, content, thr)(i)
                    staged(type_, content, thr)(i)
                torch.cuda.synchronize()
                same = same and all(torch.equal(out_f[s][t][p], out_t[s][t][p]) for s in range(S) for t in range(n) for p in range(len(dd)))
            ok = ok and same

            def timeit(fn):
                for i in range(args.warmup):
                    fn(i)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(args.reps):
                    fn(i)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e3 / args.reps

            forms = [(label, luma(t, c, thr)) for label, t, c, thr in CASES + [END]] + [("staged " + label, staged(t, c, thr)) for label, t, c, thr in CASES]
            forms += [("mix", mix), ("single", single)]
            for _, fn in forms:                         # one round of each thrown away: fresh buffers, clocks
                timeit(fn)
            times = {label: [] for label, _ in forms}
            for _ in range(args.rounds):                # interleaved rounds: all forms see the same clocks
                for label, fn in forms:
                    times[label].append(timeit(fn))
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = {k: max(v) - min(v) for k, v in times.items()}
            print("### %s over %s -> %s, %d x 1080p, unscaled, luma overlay + LUT, %d buffer sets" % (n2, n1, name, n, S))
            print("| luma | us (spread) | (a) staged, us (spread) | luma / staged | (b) mix, us (spread) | luma / mix | (c) single, us (spread) | luma / single |")
            print("|---|---|---|---|---|---|---|---|")
            verdicts = {}

            def versus(a, b):
                ahead = med[b] - med[a] > spread[b]
                behind = med[a] - med[b] > spread[b]
                verdicts["%s vs %s" % (a, b)] = {"ratio": round(med[a] / med[b], 4), "ahead": bool(ahead)}
                return "%.1f (%.1f) | %.3f, %s" % (med[b], spread[b], med[a] / med[b], "ahead" if ahead else "behind" if behind else "within the spread")
            for label, _, _, _ in CASES:
                print("| %s | %.1f (%.1f) | %s | %s | | |" % (label, med[label], spread[label], versus(label, "staged " + label), versus(label, "mix")))
            print("| %s | %.1f (%.1f) | | | %s | %s |" % (END[0], med[END[0]], spread[END[0]], versus(END[0], "mix"), versus(END[0], "single")))
            print("identical bytes (luma against staged, all nine cases): %s" % same)
            print(json.dumps({"tool": "bench_flat_luma", "layer2": n2, "layer1": n1, "format": name, "tracks": n, "us": {k: [round(x, 2) for x in v] for k, v in times.items()},
                              "median_us": {k: round(v, 2) for k, v in med.items()}, "spread_us": {k: round(v, 2) for k, v in spread.items()}, "comparisons": verdicts,
                              "identical": same}), flush=True)
            del out_f, out_t, f_trk, o_trk
        del l1, l2
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
