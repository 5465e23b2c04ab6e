#!/usr/bin/env python3
"""tools/bench_flat_chain.py -- the UNSCALED tick from decoded YUV 4:2:0 frames: 16 x 1920x1080 YUV420P tracks with chroma blend and gamma LUT -> RGBA / UYVY /
YUV420P, the decoder's frame already at the project's size.

Times, on the same data (events on the launch stream around back-to-back launches ending in a synchronise, rotated over `--sets` buffer sets so that a pass does
not sit in the 256 MiB Infinity Cache; the two forms alternated in `--rounds` rounds in the same process):
  fused -- lgpu_chain_flat_yuv420p / lgpu_chain_flat_yuv420p_to_yuv: one launch, no RGBA frame in between;
  today -- lgpu_yuv420p_to_rgb_batch into a scratch set, lgpu_chain_amounts, and for a sink lgpu_rgb_to_yuv_batch: two or three launches with the converted frame
           (and, for a sink, the finished RGBA frame) written and read back.
Prints the algorithmic bytes of each form -- per pixel 1.5 source + 4 layer 2 + the destination (4 RGBA, 2 UYVY, 1.5 YUV420P); today's form adds 4 + 4 for the
converted frame and, for a sink, 4 + 4 for the RGBA result -- per-round microseconds per tick, GB/s on those bytes, and the fused / today difference against the
round-to-round spread of today's figure: the layer seam's opt-in route (lives_gpu_set_flat_yuv) takes the fused form for a format only if the difference is
larger.  Checks that both forms give the same bytes first.  One JSON line per format.
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
    g.manual_seed(0xF1A7)
    lut = np.zeros(256, np.uint8)
    po.oracle().orc_gamma_lut8(1.0, po.GAMMA_SRGB, po.GAMMA_LINEAR, 1.4, po.P(lut))
    amounts = [int(x) for x in np.random.default_rng(0xF1A7).integers(0, 256, n)]

    def rnd(shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)

    # per set: luma, U, V and layer-2 frames of every track
    srcs = [([rnd((H, W)) for _ in range(n)], [rnd((H // 2, W // 2)) for _ in range(n)], [rnd((H // 2, W // 2)) for _ in range(n)],
             [rnd((H, W * 4)) for _ in range(n)]) for _ in range(args.sets)]
    conv = [torch.zeros((H, W * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]       # today's converted frames
    rgba = [torch.zeros((H, W * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]       # today's RGBA results in front of a sink
    prm = ops.chain_params(W, H, W * 4, W, H, W * 4, W * 4, swap_rb=0, interp=0x100, bf=0, lut=lut)
    ysrc = ops.yuv_source((W, W // 2, W // 2), H // 2 * (W // 2), H // 2 * (W // 2), out_order=0, which_tables=0, pb_quality=2)
    ok = True
    for name in args.formats.split(","):
        fmt = FMT[name]
        dd = dims(fmt)
        out_f = [[[torch.zeros((r, b), dtype=torch.uint8, device="cuda") for (b, r) in dd] for _ in range(n)] for _ in range(args.sets)]
        out_t = [[[torch.zeros((r, b), dtype=torch.uint8, device="cuda") for (b, r) in dd] for _ in range(n)] for _ in range(args.sets)]
        if fmt == 0:
            f_trk = [ops.chain_yuv_tracks(srcs[s][0], srcs[s][1], srcs[s][2], srcs[s][3], [o[0] for o in out_f[s]]) for s in range(args.sets)]
            t_trk = [ops.chain_tracks(conv, srcs[s][3], [o[0] for o in out_t[s]]) for s in range(args.sets)]
        else:
            sink = ops.chain_sink(fmt, [b for (b, _) in dd], which_tables=0, in_order=0)
            f_trk = [ops.chain_yuv_sink_tracks(srcs[s][0], srcs[s][1], srcs[s][2], srcs[s][3], out_f[s]) for s in range(args.sets)]
            t_trk = [ops.chain_tracks(conv, srcs[s][3], rgba) for s in range(args.sets)]
        frames = [list(zip(srcs[s][0], srcs[s][1], srcs[s][2], conv)) for s in range(args.sets)]

        def fused(i):
            if fmt == 0:
                ops.chain_flat_yuv420p(prm, ysrc, f_trk[i % args.sets], amounts)
            else:
                ops.chain_flat_yuv420p_to_yuv(prm, ysrc, sink, f_trk[i % args.sets], amounts)

        def today(i):
            s = i % args.sets
            ops.yuv420p_to_rgb_batch(frames[s], W, H, 4, 0, 0, 0, 2)
            ops.chain_amounts(prm, t_trk[s], amounts)
            if fmt:
                for k in range(0, n, 16):
                    ops.rgb_to_yuv_batch(rgba[k:k + 16], out_t[s][k:k + 16], W, H, 0, 1, fmt, 0, 0)

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
        bf = (W * H * 3 // 2 + W * H * 4 + dst_b) * n
        bt = bf + 2 * W * H * 4 * n * (2 if fmt else 1)
        spread = max(tt) - min(tt)
        launches = 3 if fmt else 2
        print("### %s, %d x 1080p YUV420P, unscaled, blend + LUT, %d buffer sets" % (name, n, args.sets))
        print("algorithmic bytes per pixel: fused %.2f, today %.2f" % (bf / (n * W * H), bt / (n * W * H)))
        print("| form | us per tick, median (min) | algorithmic MB per track | GB/s at the median | of 8 TB/s |")
        print("|---|---|---|---|---|")
        print("| fused (one launch) | %.1f (%.1f) | %.1f | %.0f | %.3f |" % (mf, min(tf), bf / n * 1e-6, bf / mf * 1e-3, bf / mf * 1e-3 / PEAK))
        print("| today (%d launches) | %.1f (%.1f) | %.1f | %.0f | %.3f |" % (launches, mt, min(tt), bt / n * 1e-6, bt / mt * 1e-3, bt / mt * 1e-3 / PEAK))
        print("rounds, us per tick: fused %s; today %s" % (["%.1f" % x for x in tf], ["%.1f" % x for x in tt]))
        print("fused / today at the medians: %.3f (by the bytes: %.3f); difference %.1f us; round-to-round spread of today's figure %.1f us" %
              (mf / mt, bf / bt, mt - mf, spread))
        print("identical bytes: %s" % same)
        print(json.dumps({"tool": "bench_flat_chain", "format": name, "tracks": n, "fused_us": [round(x, 2) for x in tf], "today_us": [round(x, 2) for x in tt],
                          "fused_median_us": round(mf, 2), "today_median_us": round(mt, 2), "ratio": round(mf / mt, 4), "fused_bytes": bf, "today_bytes": bt,
                          "today_spread_us": round(spread, 2), "fused_beats_today_by_more_than_spread": bool(mt - mf > spread), "identical": same}))
        del out_f, out_t, f_trk, t_trk
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
