#!/usr/bin/env python3
"""tools/bench_transcode_chain.py -- a tick from decoded YUV 4:2:0 frames to a YUV sink: 16 x 3840x2160 YUV420P tracks -> 1920x1080 with chroma blend and gamma LUT
-> YUV420P / UYVY.

Times, on the same data (events on the launch stream around back-to-back launches ending in a synchronise, rotated over `--sets` buffer sets so that a pass does
not sit in the 256 MiB Infinity Cache; the two forms alternated in `--rounds` rounds in the same process):
  fused -- lgpu_chain_yuv420p_to_yuv: K2's conversion in the chain kernel's loads and K4's in its store, one launch, no RGBA frame at either end;
  two   -- lgpu_chain_yuv420p into an RGBA scratch set + lgpu_rgb_to_yuv_batch: two launches and the 1080p RGBA result written and read back.
Prints per-round microseconds per tick, GB/s on the algorithmic bytes of each form (per track: source 12,441,600 + layer 2 8,294,400 + the sink's planes, 3,110,400
for 4:2:0 or 4,147,200 for UYVY; the two-launch form adds the RGBA frame written and read, 16,588,800) and the fused / two-launch difference against the
round-to-round spread of the two-launch figure: the layer seam takes the fused form for a format only if the difference is larger.  Checks that both forms give the
same bytes first.  One JSON line per format.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8000.0                    # GB/s
SW, SH, DW, DH = 3840, 2160, 1920, 1080
FMT = {"yuv420p": 4, "uyvy": 2, "yuyv": 3}


def dims(fmt):
    return [(DW * 2, DH)] if fmt in (2, 3) else [(DW, DH), (DW // 2, DH // 2), (DW // 2, DH // 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=16)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds of each form")
    ap.add_argument("--sets", type=int, default=3, help="buffer sets rotated between launches (cold buffers)")
    ap.add_argument("--interp", type=int, default=3, help="3 HYPER, 2 BILINEAR")
    ap.add_argument("--formats", default="yuv420p,uyvy")
    ap.add_argument("--only", choices=["fused", "two"], help="run one form alone (for a kernel trace), no timing table")
    args = ap.parse_args()
    import numpy as np
    import torch
    from lives_amd import ops
    from oracle import pyoracle as po
    ops.init(0)
    n = args.tracks
    g = torch.Generator(device="cuda")
    g.manual_seed(0x7C0DE)
    lut = np.zeros(256, np.uint8)
    po.oracle().orc_gamma_lut8(1.0, po.GAMMA_SRGB, po.GAMMA_LINEAR, 1.4, po.P(lut))
    amounts = [int(x) for x in np.random.default_rng(0x7C0DE).integers(0, 256, n)]

    def rnd(shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)

    # per set: luma, U, V and layer-2 frames of every track
    srcs = [([rnd((SH, SW)) for _ in range(n)], [rnd((SH // 2, SW // 2)) for _ in range(n)], [rnd((SH // 2, SW // 2)) for _ in range(n)],
             [rnd((DH, DW * 4)) for _ in range(n)]) for _ in range(args.sets)]
    rgba = [torch.zeros((DH, DW * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    prm = ops.chain_params(SW, SH, SW, DW, DH, DW * 4, DW * 4, swap_rb=0, interp=args.interp | 0x100, bf=0, lut=lut)
    ysrc = ops.yuv_source((SW, SW // 2, SW // 2), SH // 2 * (SW // 2), SH // 2 * (SW // 2), out_order=0, which_tables=0, pb_quality=2)
    ok = True
    for name in args.formats.split(","):
        fmt = FMT[name]
        dd = dims(fmt)
        out_f = [[[torch.zeros((r, b), dtype=torch.uint8, device="cuda") for (b, r) in dd] for _ in range(n)] for _ in range(args.sets)]
        out_t = [[[torch.zeros((r, b), dtype=torch.uint8, device="cuda") for (b, r) in dd] for _ in range(n)] for _ in range(args.sets)]
        sink = ops.chain_sink(fmt, [b for (b, _) in dd], which_tables=0, in_order=0)
        f_trk = [ops.chain_yuv_sink_tracks(srcs[s][0], srcs[s][1], srcs[s][2], srcs[s][3], out_f[s]) for s in range(args.sets)]
        t_trk = [ops.chain_yuv_tracks(srcs[s][0], srcs[s][1], srcs[s][2], srcs[s][3], rgba) for s in range(args.sets)]

        def fused(i):
            ops.chain_yuv420p_to_yuv(prm, ysrc, sink, f_trk[i % args.sets], amounts)

        def two(i):
            s = i % args.sets
            ops.chain_yuv420p(prm, ysrc, t_trk[s], amounts)
            for k in range(0, n, 16):
                ops.rgb_to_yuv_batch(rgba[k:k + 16], out_t[s][k:k + 16], DW, DH, 0, 1, fmt, 0, 0)

        if args.only:
            fn = fused if args.only == "fused" else two
            for i in range(args.warmup + args.reps):
                fn(i)
            torch.cuda.synchronize()
            continue
        for i in range(args.sets):
            fused(i)
            two(i)
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
        timeit(two)
        tf, tt = [], []
        for _ in range(args.rounds):          # interleaved rounds: both forms see the same clocks
            tf.append(timeit(fused))
            tt.append(timeit(two))
        mf, mt = statistics.median(tf), statistics.median(tt)
        sink_b = sum(b * r for (b, r) in dd)
        bf = (SW * SH * 3 // 2 + DW * DH * 4 + sink_b) * n
        bt = bf + 2 * DW * DH * 4 * n
        spread = max(tt) - min(tt)
        print("### %s, %d x 4K YUV420P -> 1080p, blend + LUT, interp %d, %d buffer sets" % (name, n, args.interp, args.sets))
        print("| form | us per tick, median (min) | algorithmic MB per track | GB/s at the median | of 8 TB/s |")
        print("|---|---|---|---|---|")
        print("| lgpu_chain_yuv420p_to_yuv (one launch) | %.1f (%.1f) | %.1f | %.0f | %.3f |" % (mf, min(tf), bf / n * 1e-6, bf / mf * 1e-3, bf / mf * 1e-3 / PEAK))
        print("| lgpu_chain_yuv420p + lgpu_rgb_to_yuv_batch | %.1f (%.1f) | %.1f | %.0f | %.3f |" % (mt, min(tt), bt / n * 1e-6, bt / mt * 1e-3, bt / mt * 1e-3 / PEAK))
        print("rounds, us per tick: fused %s; two-launch %s" % (["%.1f" % x for x in tf], ["%.1f" % x for x in tt]))
        print("fused / two-launch at the medians: %.3f (by the bytes: %.3f); difference %.1f us; round-to-round spread of the two-launch figure %.1f us" %
              (mf / mt, bf / bt, mt - mf, spread))
        print("identical bytes: %s" % same)
        print(json.dumps({"tool": "bench_transcode_chain", "format": name, "tracks": n, "interp": args.interp, "fused_us": [round(x, 2) for x in tf],
                          "two_launch_us": [round(x, 2) for x in tt], "fused_median_us": round(mf, 2), "two_launch_median_us": round(mt, 2), "ratio": round(mf / mt, 4),
                          "two_launch_spread_us": round(spread, 2), "fused_beats_two_by_more_than_spread": bool(mt - mf > spread), "identical": same}))
        del out_f, out_t, f_trk, t_trk
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
