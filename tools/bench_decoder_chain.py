#!/usr/bin/env python3
"""tools/bench_decoder_chain.py -- a tick that starts at the decoder's frames: 16 x 3840x2160 YUV420P tracks -> 1920x1080 with chroma blend and gamma LUT.

Times, on the same data (events on the launch stream around back-to-back launches, rotated over `--sets` buffer sets so that a pass does not sit in the
256 MiB Infinity Cache):
  fused -- lgpu_chain_yuv420p: the conversion in registers, one launch;
  two   -- lgpu_yuv420p_to_rgb_batch into an RGBA scratch set + lgpu_chain_amounts: two launches and the RGBA intermediate written and read back.
Prints per-launch microseconds and the fraction of 8 TB/s on the algorithmic bytes of the fused form: 4:2:0 source 12,441,600 + layer 2 8,294,400 + destination
8,294,400 = 29,030,400 B per track.  Checks that both forms give the same bytes first.  One JSON line for that part.
Then the same tracks through the layer seam: pinned YUV420P layers, the reference's calls on one host thread per track, one lives_gpu_layers_flush per tick.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8000.0                    # GB/s
SW, SH, DW, DH = 3840, 2160, 1920, 1080
BYTES_PER_TRACK = SW * SH * 3 // 2 + 2 * DW * DH * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=16)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sets", type=int, default=2, help="buffer sets rotated between launches (cold buffers)")
    ap.add_argument("--interp", type=int, default=3, help="3 HYPER, 2 BILINEAR")
    ap.add_argument("--no-seam", action="store_true", help="skip the pass through the layer seam")
    args = ap.parse_args()
    import numpy as np
    import torch
    from lives_amd import ops
    from oracle import pyoracle as po
    ops.init(0)
    n = args.tracks
    g = torch.Generator(device="cuda")
    g.manual_seed(0xDEC0)
    lut = np.zeros(256, np.uint8)
    po.oracle().orc_gamma_lut8(1.0, po.GAMMA_SRGB, po.GAMMA_LINEAR, 1.4, po.P(lut))
    amounts = [int(x) for x in np.random.default_rng(0xDEC0).integers(0, 256, n)]

    def rnd(shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)

    sets = []
    for _ in range(args.sets):
        Y = [rnd((SH, SW)) for _ in range(n)]
        U = [rnd((SH // 2, SW // 2)) for _ in range(n)]
        V = [rnd((SH // 2, SW // 2)) for _ in range(n)]
        L2 = [rnd((DH, DW * 4)) for _ in range(n)]
        D1 = [torch.zeros((DH, DW * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
        D2 = [torch.zeros((DH, DW * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
        sets.append((Y, U, V, L2, D1, D2))
    rgba = [torch.zeros((SH, SW * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    prm = ops.chain_params(SW, SH, SW * 4, DW, DH, DW * 4, DW * 4, swap_rb=0, interp=args.interp | 0x100, bf=0, lut=lut)
    src = ops.yuv_source((SW, SW // 2, SW // 2), (SW // 2) * (SH // 2), (SW // 2) * (SH // 2))
    fused_trk = [ops.chain_yuv_tracks(s[0], s[1], s[2], s[3], s[4]) for s in sets]
    frames = [[(s[0][i], s[1][i], s[2][i], rgba[i]) for i in range(n)] for s in sets]
    two_trk = [ops.chain_tracks(rgba, s[3], s[5]) for s in sets]

    def fused(i):
        ops.chain_yuv420p(prm, src, fused_trk[i % args.sets], amounts)

    def two(i):
        ops.yuv420p_to_rgb_batch(frames[i % args.sets], SW, SH)
        ops.chain_amounts(prm, two_trk[i % args.sets], amounts)

    for i in range(args.sets):
        fused(i)
        two(i)
    torch.cuda.synchronize()
    same = all(torch.equal(s[4][t], s[5][t]) for s in sets for t in range(n))

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

    # interleaved rounds: both forms see the same clocks
    tf, tt = [], []
    for _ in range(3):
        tf.append(timeit(fused))
        tt.append(timeit(two))
    uf, ut = min(tf), min(tt)
    total = BYTES_PER_TRACK * n
    print("| form | us per tick (%d x 4K 4:2:0 -> 1080p) | GB/s on %d B per track | of 8 TB/s |" % (n, BYTES_PER_TRACK))
    print("|---|---|---|---|")
    for name, us in (("lgpu_chain_yuv420p (one launch)", uf), ("lgpu_yuv420p_to_rgb_batch + lgpu_chain_amounts", ut)):
        print("| %s | %.1f | %.0f | %.3f |" % (name, us, total / us * 1e-3, total / us * 1e-3 / PEAK))
    print("fused / two-launch: %.3f   (rounds: fused %s, two %s)" % (uf / ut, ["%.1f" % x for x in tf], ["%.1f" % x for x in tt]))
    print("identical bytes: %s" % same)
    print(json.dumps({"tool": "bench_decoder_chain", "tracks": n, "interp": args.interp, "fused_us": round(uf, 2), "two_launch_us": round(ut, 2),
                      "ratio": round(uf / ut, 4), "fused_frac_of_8TBs": round(total / uf * 1e-3 / PEAK, 4), "identical": same}))
    if not args.no_seam:
        seam(args, n, np, torch)
    return 0 if same else 1


def seam(args, n, np, torch):
    """the same 16 tracks as pinned YUV420P layers through the reference's calls (convert_layer_palette -> resize_layer -> "chroma blend" -> gamma_convert_layer, one
    host thread per track), one lives_gpu_layers_flush per tick: frames/s and the deferred counters per tick"""
    import ctypes
    import threading
    import time
    from lives_amd import lib
    from oracle import pyoracle as po
    if not po.have_ref():
        print("seam: skipped (oracle/_ref, the reference libweed the host side needs, is not built)")
        return
    from tests import weedhost as wh
    L = lib.load()
    wh.bind(L)
    L.lives_gpu_layers_flush.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
    L.lives_gpu_deferred_stats_n.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    L.lives_gpu_deferred_stats_n.restype = None
    H = po.RefHost()
    fx = os.path.join(ROOT, "lives_amd", "livesgpu_fx.so")
    rng = np.random.default_rng(0x5EA)
    Y = [rng.integers(0, 256, (SH, SW), dtype=np.uint8) for _ in range(n)]
    U = [rng.integers(0, 256, (SH // 2, SW // 2), dtype=np.uint8) for _ in range(n)]
    V = [rng.integers(0, 256, (SH // 2, SW // 2), dtype=np.uint8) for _ in range(n)]
    L2 = [rng.integers(0, 256, (DH, DW * 4), dtype=np.uint8) for _ in range(n)]

    def stats():
        a = (ctypes.c_ulonglong * 8)()
        L.lives_gpu_deferred_stats_n(a, 8)
        return list(a)

    def view(layer):
        _, ptrs, rs = wh.planes_of(layer)
        return np.frombuffer((ctypes.c_uint8 * (rs[0] * DH)).from_address(ptrs[0]), np.uint8).reshape(DH, rs[0])

    l2l = [wh.new_layer(3, DW, DH, [a], gamma=1) for a in L2]
    for a in l2l:
        assert L.lives_gpu_layer_pin(a) == 0
    ticks = max(3, args.reps // 4)
    times, deltas = [], []
    for t in range(ticks + 1):
        lays = [wh.new_layer(512, SW, SH, [Y[i], U[i], V[i]], gamma=1, clamping=0, subspace=1) for i in range(n)]
        for a in lays:
            assert L.lives_gpu_layer_pin(a) == 0          # the decoder frame's upload: before the tick starts
        torch.cuda.synchronize()
        s0 = stats()
        t0 = time.perf_counter()

        def track(i):
            lay = lays[i]
            assert L.lives_gpu_convert_layer_palette(lay, 3, 0) == 1
            assert L.lives_gpu_resize_layer(lay, DW, DH, 3, 3, 0) == 1
            v, v2 = view(lay), view(l2l[i])
            H.run(fx, "chroma blend", 3, DW, DH, [v, v2], v, [po.p_int(40 + 13 * i)])
            assert L.lives_gpu_gamma_convert_layer(2, lay) == 1
        ths = [threading.Thread(target=track, args=(i,)) for i in range(n)]
        [x.start() for x in ths]
        [x.join() for x in ths]
        assert L.lives_gpu_layers_flush((ctypes.c_void_p * n)(*lays), n) == 0
        torch.cuda.synchronize()
        if t:
            times.append(time.perf_counter() - t0)
            deltas.append([b - a for a, b in zip(s0, stats())])
        for a in lays:
            assert L.lives_gpu_layer_forget(a) == 0
    for a in l2l:
        assert L.lives_gpu_layer_unpin(a) == 0
    best = min(times)
    print("seam: %d ticks of %d pinned YUV420P 4K tracks through convert_layer_palette -> resize_layer -> chroma blend -> gamma_convert_layer + one flush" % (ticks, n))
    print("seam: best tick %.2f ms = %.0f frames/s (median %.2f ms; host threads included, the uploads before the tick not)" % (best * 1e3, n / best, sorted(times)[len(times) // 2] * 1e3))
    print("seam: counter deltas per tick [recorded, chain launches, tracks, staged, yuv recorded, yuv launches, yuv tracks, pre-launches]: %s" % deltas[-1])


if __name__ == "__main__":
    sys.exit(main())
