#!/usr/bin/env python3
"""tools/bench_sink_chain.py -- a tick that ends at a YUV sink: 16 x 3840x2160 RGBA tracks -> 1920x1080 with chroma blend and gamma LUT -> YUV420P / UYVY.

Times, on the same data (events on the launch stream around back-to-back launches ending in a synchronise, rotated over `--sets` buffer sets so that a pass does
not sit in the 256 MiB Infinity Cache; the two forms alternated in three rounds in the same process):
  fused -- lgpu_chain_to_yuv: K4's conversion in the chain kernel's store, one launch, no RGBA frame;
  two   -- lgpu_chain_amounts into an RGBA scratch set + lgpu_rgb_to_yuv_batch: two launches and the RGBA result written and read back.
Prints per-tick microseconds, GB/s on the algorithmic bytes of each form (per track: source 33,177,600 + layer 2 8,294,400 + the sink's planes, 3,110,400 for
4:2:0 or 4,147,200 for UYVY; the two-launch form adds the RGBA frame written and read, 16,588,800) and the fused / two-launch ratio with the spread between the
rounds.  Checks that both forms give the same bytes first.  One JSON line per format.
"""
import argparse
import json
import os
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
    ap.add_argument("--sets", type=int, default=2, help="buffer sets rotated between launches (cold buffers)")
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
    g.manual_seed(0x51CC)
    lut = np.zeros(256, np.uint8)
    po.oracle().orc_gamma_lut8(1.0, po.GAMMA_SRGB, po.GAMMA_LINEAR, 1.4, po.P(lut))
    amounts = [int(x) for x in np.random.default_rng(0x51CC).integers(0, 256, n)]

    def rnd(shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)

    srcs = [([rnd((SH, SW * 4)) for _ in range(n)], [rnd((DH, DW * 4)) for _ in range(n)]) for _ in range(args.sets)]
    rgba = [torch.zeros((DH, DW * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    prm = ops.chain_params(SW, SH, SW * 4, DW, DH, DW * 4, DW * 4, swap_rb=1, interp=args.interp | 0x100, bf=0, lut=lut)
    ok = True
    for name in args.formats.split(","):
        fmt = FMT[name]
        dd = dims(fmt)
        out_f = [[[torch.zeros((r, b), dtype=torch.uint8, device="cuda") for (b, r) in dd] for _ in range(n)] for _ in range(args.sets)]
        out_t = [[[torch.zeros((r, b), dtype=torch.uint8, device="cuda") for (b, r) in dd] for _ in range(n)] for _ in range(args.sets)]
        sink = ops.chain_sink(fmt, [b for (b, _) in dd], which_tables=0, in_order=0)
        f_trk = [ops.chain_sink_tracks(srcs[s][0], srcs[s][1], out_f[s]) for s in range(args.sets)]
        t_trk = [ops.chain_tracks(srcs[s][0], srcs[s][1], rgba) for s in range(args.sets)]

        def fused(i):
            ops.chain_to_yuv(prm, sink, f_trk[i % args.sets], amounts)

        def two(i):
            s = i % args.sets
            ops.chain_amounts(prm, t_trk[s], amounts)
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
        for _ in range(3):          # interleaved rounds: both forms see the same clocks
            tf.append(timeit(fused))
            tt.append(timeit(two))
        uf, ut = min(tf), min(tt)
        sink_b = sum(b * r for (b, r) in dd)
        bf = (SW * SH * 4 + DW * DH * 4 + sink_b) * n
        bt = bf + 2 * DW * DH * 4 * n
        spread = max(max(tf) - min(tf), max(tt) - min(tt))
        print("### %s, %d x 4K -> 1080p, blend + LUT, interp %d" % (name, n, args.interp))
        print("| form | us per tick | algorithmic MB per track | GB/s | of 8 TB/s |")
        print("|---|---|---|---|---|")
        print("| lgpu_chain_to_yuv (one launch) | %.1f | %.1f | %.0f | %.3f |" % (uf, bf / n * 1e-6, bf / uf * 1e-3, bf / uf * 1e-3 / PEAK))
        print("| lgpu_chain_amounts + lgpu_rgb_to_yuv_batch | %.1f | %.1f | %.0f | %.3f |" % (ut, bt / n * 1e-6, bt / ut * 1e-3, bt / ut * 1e-3 / PEAK))
        print("fused / two-launch: %.3f (by the bytes: %.3f); rounds: fused %s, two-launch %s us; spread between rounds %.1f us; difference %.1f us" %
              (uf / ut, bf / bt, ["%.1f" % x for x in tf], ["%.1f" % x for x in tt], spread, ut - uf))
        print("identical bytes: %s" % same)
        print(json.dumps({"tool": "bench_sink_chain", "format": name, "tracks": n, "interp": args.interp, "fused_us": round(uf, 2), "two_launch_us": round(ut, 2),
                          "ratio": round(uf / ut, 4), "spread_us": round(spread, 2), "fused_faster_than_spread": bool(ut - uf > spread), "identical": same}))
        del out_f, out_t, f_trk, t_trk
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
