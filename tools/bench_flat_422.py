#!/usr/bin/env python3
"""tools/bench_flat_422.py -- the UNSCALED tick from 4:2:2 frames: 16 x 1920x1080 YUV422P (MJPEG, DV) or UYVY (capture) tracks with chroma blend and gamma LUT ->
RGBA / UYVY / YUV420P, the frame already at the project's size.

Times, on the same data (events on the launch stream around back-to-back launches ending in a synchronise, rotated over `--sets` buffer sets so that a pass does
not sit in the 256 MiB Infinity Cache; the two forms alternated in `--rounds` rounds in the same process):
  fused -- lgpu_chain_flat_yuv422: one launch, no RGBA frame in between;
  today -- lgpu_yuv420p_to_rgb_batch (is_422) or lgpu_yuv_to_rgb_batch into a scratch set, lgpu_chain_amounts, and for a sink lgpu_rgb_to_yuv_batch: two or three
           launches (the packed conversions go 16 frames per call) with the converted frame (and, for a sink, the finished RGBA frame) written and read back.
Prints the algorithmic bytes of each form -- per pixel 2 source + 4 layer 2 + the destination (4 RGBA, 2 UYVY, 1.5 YUV420P); today's form adds 4 + 4 for the
converted frame and, for a sink, 4 + 4 for the RGBA result -- per-round microseconds per tick, GB/s on those bytes, and the fused / today difference against the
round-to-round spread of both figures: a default may follow the fused form for a (source, destination) pair only if the difference is larger.  Checks that both
forms give the same bytes first.  One JSON line per pair.
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
SRC = {"yuv422p": 5, "uyvy": 2, "yuyv": 3}


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
    ap.add_argument("--sources", default="yuv422p,uyvy")
    ap.add_argument("--formats", default="rgba,uyvy,yuv420p")
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

    def rnd(shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)

    l2 = [[rnd((H, W * 4)) for _ in range(n)] for _ in range(args.sets)]
    conv = [torch.zeros((H, W * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]       # today's converted frames
    rgba = [torch.zeros((H, W * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]       # today's RGBA results in front of a sink
    prm = ops.chain_params(W, H, W * 4, W, H, W * 4, W * 4, swap_rb=0, interp=0x100, bf=0, lut=lut)
    ok = True
    for sname in args.sources.split(","):
        sfmt = SRC[sname]
        planar = sfmt == 5
        if planar:
            srcs = [([rnd((H, W)) for _ in range(n)], [rnd((H, W // 2)) for _ in range(n)], [rnd((H, W // 2)) for _ in range(n)]) for _ in range(args.sets)]
            ysrc = ops.yuv422_source(5, (W, W // 2, W // 2), H * (W // 2), H * (W // 2), out_order=0, which_tables=0, pb_quality=2)
        else:
            srcs = [([rnd((H, W * 2)) for _ in range(n)], None, None) for _ in range(args.sets)]
            ysrc = ops.yuv422_source(sfmt, (W * 2,), out_order=0, which_tables=0)
        for name in args.formats.split(","):
            fmt = FMT[name]
            dd = dims(fmt)
            out_f = [[[torch.zeros((r, b), dtype=torch.uint8, device="cuda") for (b, r) in dd] for _ in range(n)] for _ in range(args.sets)]
            out_t = [[[torch.zeros((r, b), dtype=torch.uint8, device="cuda") for (b, r) in dd] for _ in range(n)] for _ in range(args.sets)]
            sink = ops.chain_sink(fmt, [b for (b, _) in dd], which_tables=0, in_order=0) if fmt else None
            f_trk = [ops.chain_yuv_sink_tracks(srcs[s][0], srcs[s][1], srcs[s][2], l2[s], out_f[s]) for s in range(args.sets)]
            t_trk = [ops.chain_tracks(conv, l2[s], rgba if fmt else [o[0] for o in out_t[s]]) for s in range(args.sets)]
            frames = [list(zip(srcs[s][0], srcs[s][1], srcs[s][2], conv)) for s in range(args.sets)] if planar else None

            def fused(i):
                ops.chain_flat_yuv422(prm, ysrc, f_trk[i % args.sets], amounts, sink=sink)

            def today(i):
                s = i % args.sets
                if planar:
                    ops.yuv420p_to_rgb_batch(frames[s], W, H, 4, 0, 1, 0, 2)
                else:
                    for k in range(0, n, 16):
                        ops.yuv_to_rgb_batch([[f] for f in srcs[s][0][k:k + 16]], conv[k:k + 16], W, H, sfmt, 0, 0, 1, 0)
                ops.chain_amounts(prm, t_trk[s], amounts)
                if fmt:
                    for k in range(0, n, 16):
                        ops.rgb_to_yuv_batch(rgba[k:k + 16], out_t[s][k:k + 16], W, H, 0, 1, fmt, 0, 0)

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
            bf = (W * H * 2 + W * H * 4 + dst_b) * n
            bt = bf + 2 * W * H * 4 * n * (2 if fmt else 1)
            sp_f, sp_t = max(tf) - min(tf), max(tt) - min(tt)
            launches = (3 if fmt else 2) + (0 if planar else (n - 1) // 16)
            print("### %s -> %s, %d x 1080p, unscaled, blend + LUT, %d buffer sets" % (sname, name, n, args.sets))
            print("algorithmic bytes per pixel: fused %.2f, today %.2f" % (bf / (n * W * H), bt / (n * W * H)))
            print("| form | us per tick, median (min) | spread | algorithmic MB per track | GB/s at the median | of 8 TB/s |")
            print("|---|---|---|---|---|---|")
            print("| fused (one launch) | %.1f (%.1f) | %.1f | %.1f | %.0f | %.3f |" % (mf, min(tf), sp_f, bf / n * 1e-6, bf / mf * 1e-3, bf / mf * 1e-3 / PEAK))
            print("| today (%d launches) | %.1f (%.1f) | %.1f | %.1f | %.0f | %.3f |" % (launches, mt, min(tt), sp_t, bt / n * 1e-6, bt / mt * 1e-3, bt / mt * 1e-3 / PEAK))
            print("rounds, us per tick: fused %s; today %s" % (["%.1f" % x for x in tf], ["%.1f" % x for x in tt]))
            print("fused / today at the medians: %.3f (by the bytes: %.3f); difference %.1f us; round-to-round spread: fused %.1f us, today %.1f us" %
                  (mf / mt, bf / bt, mt - mf, sp_f, sp_t))
            print("identical bytes: %s" % same)
            print(json.dumps({"tool": "bench_flat_422", "source": sname, "format": name, "tracks": n, "fused_us": [round(x, 2) for x in tf],
                              "today_us": [round(x, 2) for x in tt], "fused_median_us": round(mf, 2), "today_median_us": round(mt, 2), "ratio": round(mf / mt, 4),
                              "fused_bytes": bf, "today_bytes": bt, "fused_spread_us": round(sp_f, 2), "today_spread_us": round(sp_t, 2),
                              "fused_beats_today_by_more_than_spread": bool(mt - mf > max(sp_f, sp_t)), "identical": same}))
            del out_f, out_t, f_trk, t_trk
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
