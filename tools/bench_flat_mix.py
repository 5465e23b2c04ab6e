#!/usr/bin/env python3
"""tools/bench_flat_mix.py -- the unscaled tick that mixes TWO decoded YUV 4:2:0 clips: 16 x 1920x1080 tracks, both layers YUV420P at the project's size, chroma blend
and gamma LUT -> RGBA / UYVY / YUV420P.

Times, on the same data (events on the launch stream around back-to-back launches ending in a synchronise, rotated over `--sets` buffer sets so that a pass does
not sit in the 256 MiB Infinity Cache; the two forms alternated in `--rounds` rounds in the same process):
  fused -- lgpu_chain_flat_yuv420p_mix: one launch, both K2 conversions in the loads, no RGBA frame anywhere;
  today -- lgpu_yuv420p_to_rgb_batch on the layer-2 planes into scratch frames, then lgpu_chain_flat_yuv420p / lgpu_chain_flat_yuv420p_to_yuv reading them back: two
           launches, 4 bytes per pixel written and 4 read in between.  This is the yardstick; it runs no code of the fused form.
Prints the algorithmic bytes of each form -- per pixel 1.5 + 1.5 source + the destination (4 RGBA, 2 UYVY, 1.5 YUV420P); today's form 1.5 + 4 for the conversion and
1.5 + 4 + the destination for the chain -- per-round microseconds per tick, GB/s on those bytes, and the fused / today difference against the round-to-round spread
of today's figure (the project's criterion: won when the one launch beats today's form by more than that spread).  Checks that both forms give the same bytes
first.  One JSON line per format.  Reads nothing outside the tree.
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
FMT = {"rgba": 0, "yuv420p": 4, "uyvy": 2, "yuyv": 3}


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
    ap.add_argument("--only", choices=["fused", "today"], help="run one form alone (for a kernel trace), no timing table")
    args = ap.parse_args()
    import numpy as np
    import torch
    from lives_amd import ops
    from oracle import pyoracle as po
    ops.init(0)
    n = args.tracks
    g = torch.Generator(device="cuda")
    g.manual_seed(0x313)
    lut = np.zeros(256, np.uint8)
    po.oracle().orc_gamma_lut8(1.0, po.GAMMA_SRGB, po.GAMMA_LINEAR, 1.4, po.P(lut))
    amounts = [int(x) for x in np.random.default_rng(0x313).integers(0, 256, n)]

    def rnd(shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)

    def clip():
        return [rnd((H, W)) for _ in range(n)], [rnd((H // 2, W // 2)) for _ in range(n)], [rnd((H // 2, W // 2)) for _ in range(n)]

    # per set: luma, U, V of every track's layer 1 and of its layer 2
    l1 = [clip() for _ in range(args.sets)]
    l2 = [clip() for _ in range(args.sets)]
    conv = [torch.zeros((H, W * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]       # today's converted layer-2 frames
    prm = ops.chain_params(W, H, W * 4, W, H, W * 4, W * 4, swap_rb=0, interp=0x100, bf=0, lut=lut)
    ysrc = ops.yuv_source((W, W // 2, W // 2), H // 2 * (W // 2), H // 2 * (W // 2), out_order=0, which_tables=0, pb_quality=2)
    ok = True
    for name in args.formats.split(","):
        fmt = FMT[name]
        dd = dims(fmt)
        out_f = [[[torch.zeros((r, b), dtype=torch.uint8, device="cuda") for (b, r) in dd] for _ in range(n)] for _ in range(args.sets)]
        out_t = [[[torch.zeros((r, b), dtype=torch.uint8, device="cuda") for (b, r) in dd] for _ in range(n)] for _ in range(args.sets)]
        sink = ops.chain_sink(fmt, [b for (b, _) in dd], which_tables=0, in_order=0) if fmt else None
        f_trk = [ops.chain_yuv_mix_tracks(l1[s][0], l1[s][1], l1[s][2], l2[s][0], l2[s][1], l2[s][2], out_f[s]) for s in range(args.sets)]
        if fmt == 0:
            t_trk = [ops.chain_yuv_tracks(l1[s][0], l1[s][1], l1[s][2], conv, [o[0] for o in out_t[s]]) for s in range(args.sets)]
        else:
            t_trk = [ops.chain_yuv_sink_tracks(l1[s][0], l1[s][1], l1[s][2], conv, out_t[s]) for s in range(args.sets)]
        frames = [list(zip(l2[s][0], l2[s][1], l2[s][2], conv)) for s in range(args.sets)]

        def fused(i):
            ops.chain_flat_yuv420p_mix(prm, ysrc, ysrc, f_trk[i % args.sets], amounts, sink=sink)

        def today(i):
            s = i % args.sets
            ops.yuv420p_to_rgb_batch(frames[s], W, H, 4, 0, 0, 0, 2)
            if fmt == 0:
                ops.chain_flat_yuv420p(prm, ysrc, t_trk[s], amounts)
            else:
                ops.chain_flat_yuv420p_to_yuv(prm, ysrc, sink, t_trk[s], amounts)

        if args.only:
            fn = fused if args.only == "fused" else today
            for i in range(args.warmup + args.reps):
                fn(i)
            torch.cuda.synchronize()
            continue
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
        bf = (2 * (W * H * 3 // 2) + dst_b) * n
        bt = bf + 2 * W * H * 4 * n
        spread = max(tt) - min(tt)
        print("### %s, %d x 1080p, both layers YUV420P, unscaled, blend + LUT, %d buffer sets" % (name, n, args.sets))
        print("algorithmic bytes per pixel: fused %.2f, today %.2f" % (bf / (n * W * H), bt / (n * W * H)))
        print("| form | us per tick, median (min) | algorithmic MB per track | GB/s at the median | of 8 TB/s |")
        print("|---|---|---|---|---|")
        print("| fused (one launch) | %.1f (%.1f) | %.1f | %.0f | %.3f |" % (mf, min(tf), bf / n * 1e-6, bf / mf * 1e-3, bf / mf * 1e-3 / PEAK))
        print("| today (2 launches) | %.1f (%.1f) | %.1f | %.0f | %.3f |" % (mt, min(tt), bt / n * 1e-6, bt / mt * 1e-3, bt / mt * 1e-3 / PEAK))
        print("rounds, us per tick: fused %s; today %s" % (["%.1f" % x for x in tf], ["%.1f" % x for x in tt]))
        print("fused / today at the medians: %.3f (by the bytes: %.3f); difference %.1f us; round-to-round spread of today's figure %.1f us" %
              (mf / mt, bf / bt, mt - mf, spread))
        print("identical bytes: %s" % same)
        print(json.dumps({"tool": "bench_flat_mix", "format": name, "tracks": n, "fused_us": [round(x, 2) for x in tf], "today_us": [round(x, 2) for x in tt],
                          "fused_median_us": round(mf, 2), "today_median_us": round(mt, 2), "ratio": round(mf / mt, 4), "fused_bytes": bf, "today_bytes": bt,
                          "today_spread_us": round(spread, 2), "fused_beats_today_by_more_than_spread": bool(mt - mf > spread), "identical": same}))
        del out_f, out_t, f_trk, t_trk
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
