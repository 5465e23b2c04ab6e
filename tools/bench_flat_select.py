#!/usr/bin/env python3
"""tools/bench_flat_select.py -- a select transition between two decoded clips in one launch (lgpu_chain_flat_yuv_select, include/lives_gpu_select.h): 16 x 1920x1080
tracks with the gamma LUT, <layer 2> over <layer 1> each YUV420P, YUV422P or UYVY, to RGBA and to UYVY.

Timed, by the protocol of tools/bench_flat_mix422.py (events on the launch stream around back-to-back launches ending in a synchronise, rotated over `--sets` buffer
sets so that a pass does not sit in the 256 MiB Infinity Cache, all forms alternated in `--rounds` rounds in the same process, the round-to-round spread reported):
  select -- the one launch: iris rectangle at amounts 0, 0.5 and 1, iris circle at 0.5, dissolve at 0.5;
  (a) staged -- the launches that DEFINE the bytes, in their batch forms where they exist: both conversions (lgpu_yuv420p_to_rgb_batch / lgpu_yuv_to_rgb_batch), the
      transition (lgpu_fx_batch LGPU_FX_TRANSITION; the dissolve has no batch form: lgpu_dissolve per track), lgpu_gamma_apply_batch [, lgpu_rgb_to_yuv_batch];
  (b) mix -- lgpu_chain_flat_yuv_mix on the same pair: the crossfade, which converts both layers everywhere;
  (c) single -- against amount 0 only: layer 1's single-layer flat form with LGPU_INTERP_NOBLEND.
Checks first that select and staged give the same bytes.  No ratio is fixed in advance: the figures ship as measured, and each comparison says whether the one launch
is ahead by more than the spread of the other form's rounds.  One JSON line per pair and format.  Reads nothing outside the tree."""
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
RECT, CIRCLE, DISSOLVE = 0, 1, 3
CASES = [("rect@0", RECT, 0.0), ("rect@0.5", RECT, 0.5), ("rect@1", RECT, 1.0), ("circle@0.5", CIRCLE, 0.5), ("dissolve@0.5", DISSOLVE, 0.5)]


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
    ap.add_argument("--pairs", default="yuv420p/yuv420p,uyvy/yuv420p,yuv422p/yuv422p", help="<layer 2>/<layer 1>, comma separated")
    args = ap.parse_args()
    import numpy as np
    import torch
    from lives_amd import lib, ops
    from oracle import pyoracle as po
    ops.init(0)
    n, S = args.tracks, args.sets
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5E1)
    lut = np.zeros(256, np.uint8)
    po.oracle().orc_gamma_lut8(1.0, po.GAMMA_SRGB, po.GAMMA_LINEAR, 1.4, po.P(lut))
    masks = [torch.from_numpy(ops.dissolve_mask(0xD155 + t, W, H)).cuda() for t in range(n)]

    def rnd(r, b):
        return [torch.randint(0, 256, (r, b), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]

    def clip(f):
        """the planes of n tracks (None: the format has no such plane), their strides and chroma plane bytes"""
        if f in (2, 3):
            return [rnd(H, W * 2), None, None], (W * 2,), 0
        ch = H // 2 if f == 4 else H
        return [rnd(H, W), rnd(ch, W // 2), rnd(ch, W // 2)], (W, W // 2, W // 2), ch * (W // 2)

    ca = [torch.zeros((H, W * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]       # the staged form's converted layers and its RGBA result
    cb = [torch.zeros((H, W * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    res = [torch.zeros((H, W * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    res_p = (ctypes.c_void_p * n)(*[t.data_ptr() for t in res])
    prm = ops.chain_params(W, H, W * 4, W, H, W * 4, W * 4, swap_rb=0, interp=0x100, bf=0, lut=lut)
    prm_single = ops.chain_params(W, H, W * 4, W, H, W * 4, W * 4, swap_rb=0, interp=0x100 | 0x400, bf=0, lut=lut)
    ok = True
    for pair in args.pairs.split(","):
        n2, n1 = pair.split("/")
        f2, f1 = FMT[n2], FMT[n1]
        l1, l2 = [clip(f1) for _ in range(S)], [clip(f2) for _ in range(S)]
        (_, st1, csz1), (_, st2, csz2) = l1[0], l2[0]
        s1 = ops.yuv_layer_source(f1, st1, csz1, csz1, out_order=0, which_tables=0, pb_quality=2)
        s2 = ops.yuv_layer_source(f2, st2, csz2, csz2, out_order=0, which_tables=0, pb_quality=2)
        old1 = ops.yuv_source(st1, csz1, csz1, out_order=0, which_tables=0, pb_quality=2) if f1 == 4 else ops.yuv422_source(f1, st1, csz1, csz1, out_order=0, which_tables=0, pb_quality=2)
        for name in args.formats.split(","):
            fmt = FMT[name]
            dd = dims(fmt)
            new = lambda: [[[torch.zeros((r, b), dtype=torch.uint8, device="cuda") for (b, r) in dd] for _ in range(n)] for _ in range(S)]
            out_f, out_t = new(), new()
            sink = ops.chain_sink(fmt, [b for (b, _) in dd], which_tables=0, in_order=0) if fmt else None
            f_trk = [ops.chain_yuv_mix_tracks(l1[s][0][0], l1[s][0][1], l1[s][0][2], l2[s][0][0], l2[s][0][1], l2[s][0][2], out_f[s]) for s in range(S)]
            if f1 == 4 and fmt == 0:
                o_trk = [ops.chain_yuv_tracks(l1[s][0][0], l1[s][0][1], l1[s][0][2], None, [o[0] for o in out_f[s]]) for s in range(S)]
            else:
                o_trk = [ops.chain_yuv_sink_tracks(l1[s][0][0], l1[s][0][1], l1[s][0][2], None, out_f[s]) for s in range(S)]

            def select(kind, amount):
                return lambda i: ops.chain_flat_yuv_select(prm, s1, s2, f_trk[i % S], kind, [amount] * n, masks=masks if kind == DISSOLVE else None, sink=sink)

            def convert(f, L, s, dst):
                if f in (2, 3):
                    ops.yuv_to_rgb_batch([[x] for x in L[s][0][0]], dst, W, H, f, 0, 0, 1, 0)
                else:
                    ops.yuv420p_to_rgb_batch(list(zip(L[s][0][0], L[s][0][1], L[s][0][2], dst)), W, H, 4, 0, int(f == 5), 0, 2)

            def staged(kind, amount):
                def run(i):
                    s = i % S
                    convert(f2, l2, s, cb)
                    convert(f1, l1, s, ca)
                    target = [o[0] for o in out_t[s]] if fmt == 0 else res
                    if kind == DISSOLVE:
                        for t in range(n):
                            ops.dissolve(ca[t], cb[t], target[t], W, H, 4, masks[t], amount)
                    else:
                        ops.fx_batch(ops.FX_TRANSITION, [[x] for x in ca], [[x] for x in target], W, H, ins1=[[x] for x in cb], ip=(kind, 4, 0, 0), dp=(amount, 0.))
                    tp = (ctypes.c_void_p * n)(*[t.data_ptr() for t in target])
                    lib.call("lgpu_gamma_apply_batch", tp, W * 4, 0, 0, W, H, 4, 0, ops.lut_ptr(lut)[0], n, ops.stream_ptr())
                    if fmt:
                        ops.rgb_to_yuv_batch(res, out_t[s], W, H, 0, 1, fmt, 0, 0)
                return run

            def mix(i):
                ops.chain_flat_yuv_mix(prm, s1, s2, f_trk[i % S], [128] * n, sink=sink)

            def single(i):
                if f1 != 4:
                    ops.chain_flat_yuv422(prm_single, old1, o_trk[i % S], None, sink=sink)
                elif fmt == 0:
                    ops.chain_flat_yuv420p(prm_single, old1, o_trk[i % S], None)
                else:
                    ops.chain_flat_yuv420p_to_yuv(prm_single, old1, sink, o_trk[i % S], None)

            same = True
            for label, kind, amount in CASES:          # the same bytes first
                for i in range(S):
                    select(kind, amount)(i)
                    staged(kind, amount)(i)
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

            forms = [(label, select(kind, amount)) for label, kind, amount in CASES] + [("staged " + label, staged(kind, amount)) for label, kind, amount in CASES[1:]]
            forms += [("staged rect@0", staged(RECT, 0.0)), ("mix", mix), ("single", single)]
            for _, fn in forms:                         # one round of each thrown away: fresh buffers, clocks
                timeit(fn)
            times = {label: [] for label, _ in forms}
            for _ in range(args.rounds):                # interleaved rounds: all forms see the same clocks
                for label, fn in forms:
                    times[label].append(timeit(fn))
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = {k: max(v) - min(v) for k, v in times.items()}
            print("### %s over %s -> %s, %d x 1080p, unscaled, select + LUT, %d buffer sets" % (n2, n1, name, n, S))
            print("| form | us per tick, median (min) | round-to-round spread, us |")
            print("|---|---|---|")
            for label, _ in forms:
                print("| %s | %.1f (%.1f) | %.1f |" % (label, med[label], min(times[label]), spread[label]))
            cmp_ = []
            for label, kind, amount in CASES:
                cmp_.append((label, "staged " + label))
                cmp_.append((label, "mix"))
            cmp_.append(("rect@0", "single"))
            print("| select | against | ratio at the medians | difference, us | spread of the other form, us | ahead by more than the spread |")
            print("|---|---|---|---|---|---|")
            verdicts = {}
            for a, b in cmp_:
                ahead = med[b] - med[a] > spread[b]
                verdicts["%s vs %s" % (a, b)] = {"ratio": round(med[a] / med[b], 4), "ahead": bool(ahead)}
                print("| %s | %s | %.3f | %.1f | %.1f | %s |" % (a, b, med[a] / med[b], med[b] - med[a], spread[b], "yes" if ahead else "no"))
            print("identical bytes (select against staged, all five cases): %s" % same)
            print(json.dumps({"tool": "bench_flat_select", "layer2": n2, "layer1": n1, "format": name, "tracks": n, "us": {k: [round(x, 2) for x in v] for k, v in times.items()},
                              "median_us": {k: round(v, 2) for k, v in med.items()}, "spread_us": {k: round(v, 2) for k, v in spread.items()}, "comparisons": verdicts,
                              "identical": same}), flush=True)
            del out_f, out_t, f_trk, o_trk
        del l1, l2
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
