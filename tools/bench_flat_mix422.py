#!/usr/bin/env python3
"""tools/bench_flat_mix422.py -- the unscaled tick that mixes two decoded clips of ANY decoded format: 16 x 1920x1080 tracks, each layer YUV420P, YUV422P or UYVY at
the project's size, chroma blend and gamma LUT -> RGBA / UYVY / YUV420P.

Times, on the same data (events on the launch stream around back-to-back launches ending in a synchronise, rotated over `--sets` buffer sets so that a pass does
not sit in the 256 MiB Infinity Cache; the two forms alternated in `--rounds` rounds in the same process):
  fused -- lgpu_chain_flat_yuv_mix: one launch, both conversions in the loads, no RGBA frame anywhere;
  today -- lgpu_yuv_to_rgb_batch (packed) or lgpu_yuv420p_to_rgb_batch (planar, is_422 as the format says) on layer 2 into scratch frames, then the existing flat form
           of layer 1's format (lgpu_chain_flat_yuv420p[_to_yuv] / lgpu_chain_flat_yuv422) reading them back: two launches, 4 bytes per pixel written and 4 read in
           between.  This is the yardstick; it runs no code of the fused form.
A pair is named `<layer 2> over <layer 1>`.  Prints the algorithmic bytes of each form -- per pixel 1.5 (YUV420P) or 2 (YUV422P, UYVY) for each layer + the
destination (4 RGBA, 2 UYVY, 1.5 YUV420P); today's form 8 more -- per-round microseconds per tick, GB/s on those bytes, and the fused / today difference against the
round-to-round spread of today's figure (the project's criterion: ahead when the one launch beats today's form by more than that spread).  Checks that both forms
give the same bytes first.  One JSON line per pair and format.  Reads nothing outside the tree.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8000.0                    # GB/s
W, H = 1920, 1080
FMT = {"rgba": 0, "yuv420p": 4, "uyvy": 2, "yuyv": 3, "yuv422p": 5}
BPP = {4: 1.5, 5: 2.0, 2: 2.0, 3: 2.0}


def dims(fmt):
    if fmt == 0:
        return [(W * 4, H)]
    return [(W * 2, H)] if fmt in (2, 3) else [(W, H), (W // 2, H // 2), (W // 2, H // 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=16)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds of each form")
    ap.add_argument("--sets", type=int, default=4, help="buffer sets rotated between launches (cold buffers)")
    ap.add_argument("--formats", default="rgba,uyvy,yuv420p")
    ap.add_argument("--pairs", default="uyvy/yuv420p,yuv420p/uyvy,yuv422p/yuv422p,uyvy/uyvy", help="<layer 2>/<layer 1>, comma separated")
    args = ap.parse_args()
    import numpy as np
    import torch
    from lives_amd import ops
    from oracle import pyoracle as po
    ops.init(0)
    n = args.tracks
    g = torch.Generator(device="cuda")
    g.manual_seed(0x422)
    lut = np.zeros(256, np.uint8)
    po.oracle().orc_gamma_lut8(1.0, po.GAMMA_SRGB, po.GAMMA_LINEAR, 1.4, po.P(lut))
    amounts = [int(x) for x in np.random.default_rng(0x422).integers(0, 256, n)]

    def rnd(r, b):
        return [torch.randint(0, 256, (r, b), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]

    def clip(f):
        """the planes of n tracks (None: the format has no such plane), their strides and chroma plane bytes"""
        if f in (2, 3):
            return [rnd(H, W * 2), None, None], (W * 2,), 0
        ch = H // 2 if f == 4 else H
        return [rnd(H, W), rnd(ch, W // 2), rnd(ch, W // 2)], (W, W // 2, W // 2), ch * (W // 2)

    conv = [torch.zeros((H, W * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]       # today's converted layer-2 frames
    prm = ops.chain_params(W, H, W * 4, W, H, W * 4, W * 4, swap_rb=0, interp=0x100, bf=0, lut=lut)
    ok = True
    for pair in args.pairs.split(","):
        n2, n1 = pair.split("/")
        f2, f1 = FMT[n2], FMT[n1]
        l1 = [clip(f1) for _ in range(args.sets)]
        l2 = [clip(f2) for _ in range(args.sets)]
        (_, st1, csz1), (_, st2, csz2) = l1[0], l2[0]
        s1 = ops.yuv_layer_source(f1, st1, csz1, csz1, out_order=0, which_tables=0, pb_quality=2)
        s2 = ops.yuv_layer_source(f2, st2, csz2, csz2, out_order=0, which_tables=0, pb_quality=2)
        old1 = ops.yuv_source(st1, csz1, csz1, out_order=0, which_tables=0, pb_quality=2) if f1 == 4 else ops.yuv422_source(f1, st1, csz1, csz1, out_order=0, which_tables=0, pb_quality=2)
        for name in args.formats.split(","):
            fmt = FMT[name]
            dd = dims(fmt)
            out_f = [[[torch.zeros((r, b), dtype=torch.uint8, device="cuda") for (b, r) in dd] for _ in range(n)] for _ in range(args.sets)]
            out_t = [[[torch.zeros((r, b), dtype=torch.uint8, device="cuda") for (b, r) in dd] for _ in range(n)] for _ in range(args.sets)]
            sink = ops.chain_sink(fmt, [b for (b, _) in dd], which_tables=0, in_order=0) if fmt else None
            f_trk = [ops.chain_yuv_mix_tracks(l1[s][0][0], l1[s][0][1], l1[s][0][2], l2[s][0][0], l2[s][0][1], l2[s][0][2], out_f[s]) for s in range(args.sets)]
            if f1 == 4 and fmt == 0:
                t_trk = [ops.chain_yuv_tracks(l1[s][0][0], l1[s][0][1], l1[s][0][2], conv, [o[0] for o in out_t[s]]) for s in range(args.sets)]
            else:
                t_trk = [ops.chain_yuv_sink_tracks(l1[s][0][0], l1[s][0][1], l1[s][0][2], conv, out_t[s]) for s in range(args.sets)]

            def fused(i):
                ops.chain_flat_yuv_mix(prm, s1, s2, f_trk[i % args.sets], amounts, sink=sink)

            def today(i):
                s = i % args.sets
                if f2 in (2, 3):
                    ops.yuv_to_rgb_batch([[f] for f in l2[s][0][0]], conv, W, H, f2, 0, 0, 1, 0)
                else:
                    ops.yuv420p_to_rgb_batch(list(zip(l2[s][0][0], l2[s][0][1], l2[s][0][2], conv)), W, H, 4, 0, int(f2 == 5), 0, 2)
                if f1 != 4:
                    ops.chain_flat_yuv422(prm, old1, t_trk[s], amounts, sink=sink)
                elif fmt == 0:
                    ops.chain_flat_yuv420p(prm, old1, t_trk[s], amounts)
                else:
                    ops.chain_flat_yuv420p_to_yuv(prm, old1, sink, t_trk[s], amounts)

            for i in range(args.sets):
                fused(i)
                today(i)
            torch.cuda.synchronize()
            same = all(torch.equal(out_f[s][t][p], out_t[s][t][p]) for s in range(args.sets) for t in range(n) for p in range(len(dd)))
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

            timeit(fused)               # one round of each thrown away: fresh buffers, clocks
            timeit(today)
            tf, tt = [], []
            for _ in range(args.rounds):          # interleaved rounds: both forms see the same clocks
                tf.append(timeit(fused))
                tt.append(timeit(today))
            mf, mt = statistics.median(tf), statistics.median(tt)
            dst_b = sum(b * r for (b, r) in dd)
            bf = int((BPP[f1] + BPP[f2]) * W * H + dst_b) * n
            bt = bf + 2 * W * H * 4 * n
            spread = max(tt) - min(tt)
            print("### %s over %s -> %s, %d x 1080p, unscaled, blend + LUT, %d buffer sets" % (n2, n1, name, n, args.sets))
            print("algorithmic bytes per pixel: fused %.2f, today %.2f" % (bf / (n * W * H), bt / (n * W * H)))
            print("| form | us per tick, median (min) | algorithmic MB per track | GB/s at the median | of 8 TB/s |")
            print("|---|---|---|---|---|")
            print("| fused (one launch) | %.1f (%.1f) | %.1f | %.0f | %.3f |" % (mf, min(tf), bf / n * 1e-6, bf / mf * 1e-3, bf / mf * 1e-3 / PEAK))
            print("| today (2 launches) | %.1f (%.1f) | %.1f | %.0f | %.3f |" % (mt, min(tt), bt / n * 1e-6, bt / mt * 1e-3, bt / mt * 1e-3 / PEAK))
            print("rounds, us per tick: fused %s; today %s" % (["%.1f" % x for x in tf], ["%.1f" % x for x in tt]))
            print("fused / today at the medians: %.3f (by the bytes: %.3f); difference %.1f us; round-to-round spread of today's figure %.1f us" %
                  (mf / mt, bf / bt, mt - mf, spread))
            print("identical bytes: %s" % same)
            print(json.dumps({"tool": "bench_flat_mix422", "layer2": n2, "layer1": n1, "format": name, "tracks": n, "fused_us": [round(x, 2) for x in tf],
                              "today_us": [round(x, 2) for x in tt], "fused_median_us": round(mf, 2), "today_median_us": round(mt, 2), "ratio": round(mf / mt, 4),
                              "fused_bytes": bf, "today_bytes": bt, "today_spread_us": round(spread, 2), "fused_beats_today_by_more_than_spread": bool(mt - mf > spread),
                              "identical": same}), flush=True)
            del out_f, out_t, f_trk, t_trk
        del l1, l2
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
