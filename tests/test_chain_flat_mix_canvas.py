"""lgpu_chain_flat_yuv_mix_canvas: the unscaled transition between two decoded frames of any of the four decoded formats, both LETTERBOXED onto one canvas of opaque
black, as one launch -- bars included, no RGBA frame anywhere -- against the oracle's composition of the header's three steps: layer 2 through the single-frame
conversion of its format into a tight RGBA array (tests/test_chain_flat_mix422.py's to_rgba), that array letterboxed onto opaque black at (offs_x, offs_y) (the blit
lgpu_letterbox_at is tested against in tests/test_wide_frames.py, as tests/test_chain_flat.py's oracle_flat writes it), then today's one-launch form of layer 1's format
with the canvas and that frame as layer 2 (oracle_flat for 4:2:0, tests/test_chain_flat422.py's first_stage + oracle_tail for the 4:2:2 formats).  Bit-exact: every byte
of the canvas, and every byte of the destination's row padding and guard rows, which start as random sentinel bytes.

A pair is written (layer 1's format, layer 2's format), as in tests/test_chain_flat_mix422.py."""
import ctypes

import numpy as np
import pytest

from tests.chain_ref import distinct_amounts
from tests.offset_buffers import dev_at
from tests.test_chain_flat import gamma_lut, oracle_flat
from tests.test_chain_flat422 import first_stage, oracle_tail
from tests.test_chain_flat_mix422 import (E_BADARG, E_UNSUPPORTED, GUARD, NAME, PAIRS, PIXBUF, NOBLEND, UYVY, YUYV, YUV420P, YUV422P, RGBA, case, expected_mix, layer,
                                          pair_id, packed, source_of, to_rgba, up)
from tests.util import align, host

FRAMES = [(2, 1), (2, 2), (2, 3), (4, 4), (6, 5)]          # row 0 alone; + the trailing row; + a row pair; pairs and a trailing row at two columns; three columns
INVERTED = (255 - np.arange(256)).astype(np.uint8)         # a LUT that does not keep black: a bar pixel is 255, 255, 255 under it
OFFSETS = [(0, 0), (1, 0), (0, 1), (3, 2)]                 # an odd offs_x puts every pixel pair on a 4-byte boundary only: the 4-byte store class


def extents(sw, sh):
    """the canvases that have bars on no side, and on one side only for each of the four sides: (what, (nwidth, nheight, offs_x, offs_y))"""
    return [("no bars", (sw, sh, 0, 0)), ("left", (sw + 1, sh, 1, 0)), ("right", (sw + 2, sh, 0, 0)), ("above", (sw, sh + 1, 0, 1)), ("below", (sw, sh + 2, 0, 0))]


def letterboxed(rgba, sw, sh, canvas):
    """step 1b: lgpu_letterbox_at(.., 4, {0, 0, 0, 255}, offs_x, offs_y) of a tight sw x sh RGBA frame into a tight canvas-sized one"""
    w, h, ox, oy = canvas
    big = np.zeros((h, w * 4), np.uint8)
    big[:, 3::4] = 255
    big[oy:oy + sh, ox * 4:(ox + sw) * 4] = rgba[:sh, :sw * 4]
    return big


def expected_canvas(orc, f1, f2, fr1, fr2, L1, L2, sw, sh, order, swap, amount, lut, canvas):
    """the three steps of the header for one track: the canvas-sized RGBA frame"""
    l2 = letterboxed(to_rgba(orc, f2, fr2, sw, sh, order ^ swap, L2), sw, sh, canvas)
    pl, st = fr1
    if f1 == YUV420P:
        return oracle_flat(orc, pl[0], pl[1], pl[2], st, sw, sh, order, swap, L1["wt"], L1["q"], L1["fix"], l2, amount, lut, canvas, RGBA, 0)[0]
    rgba = first_stage(orc, f1, pl, st, sw, sh, order, L1["wt"], L1["q"])
    return oracle_tail(orc, rgba, sw, sh, order, swap, l2, amount, lut, canvas, RGBA, 0)[0]


def run(gpu, orc, c, canvas, lut=None, order=0, swap=0, pad=8, dst_off=0):
    """one call on the frames of c (tests/test_chain_flat_mix422.py's case()): every track differs, the device buffers are allocated in a shuffled order and handed over in
    another.  The destination is canvas-sized plus row padding and guard rows, all sentinel bytes first; it is compared whole"""
    ops = gpu
    f1, f2, sw, sh, n, L1, L2, amounts = c["f1"], c["f2"], c["sw"], c["sh"], c["ntracks"], c["L1"], c["L2"], c["amounts"]
    rng = np.random.default_rng([int(v) for v in np.atleast_1d(c["seed"])] + [2])
    cw, ch = canvas[0], canvas[1]
    stride = align(cw * 4 + pad, 4)
    fills = [rng.integers(0, 256, (ch + GUARD, stride), dtype=np.uint8) for _ in range(n)]
    d1, d2, dd = [None] * n, [None] * n, [None] * n
    for i in rng.permutation(n):
        dd[i] = dev_at(fills[i], dst_off)
        d2[i] = [up(p) for p in c["frames2"][i][0]]
        d1[i] = [up(p) for p in c["frames"][i][0]]
    slots = [int(k) for k in rng.permutation(n)]
    prm = ops.chain_params(sw, sh, 0, sw, sh, 0, stride, swap_rb=swap, interp=PIXBUF, bf=0, lut=lut)
    src, src2 = source_of(ops, f1, c["frames"][0], L1, order), source_of(ops, f2, c["frames2"][0], L2, order ^ swap)

    def chroma(d, f, j):
        return [d[k][j] for k in slots] if not packed(f) else None
    trk = ops.chain_yuv_mix_tracks([d1[k][0] for k in slots], chroma(d1, f1, 1), chroma(d1, f1, 2), [d2[k][0] for k in slots], chroma(d2, f2, 1), chroma(d2, f2, 2),
                                   [[dd[k]] for k in slots])
    ops.chain_flat_yuv_mix_canvas(prm, src, src2, trk, [amounts[k] for k in slots], canvas=canvas)
    for i in range(n):
        want = expected_canvas(orc, f1, f2, c["frames"][i], c["frames2"][i], L1, L2, sw, sh, order, swap, amounts[i], lut, canvas)
        got = host(dd[i])
        bad = got[:ch, :cw * 4] != want[:ch, :cw * 4]
        assert not bad.any(), "%s over %s, %dx%d on %s, track %d: %d bytes differ from the oracle, first at %s" % (
            NAME[f2], NAME[f1], sw, sh, canvas, i, int(bad.sum()), np.argwhere(bad)[0].tolist())
        assert (got[:ch, cw * 4:] == fills[i][:ch, cw * 4:]).all(), "track %d: row padding was written" % i
        assert (got[ch:] == fills[i][ch:]).all(), "track %d: guard rows were written" % i


def packed_as(f, yuyv):
    return YUYV if yuyv and packed(f) else f


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_mix_canvas_symbol_and_wrapper():
    """the entry point in the built library, with the eight arguments of include/lives_gpu.h"""
    from lives_amd import lib, ops
    assert len(lib.PROTOTYPES["lgpu_chain_flat_yuv_mix_canvas"]) == 8
    assert hasattr(lib.load(), "lgpu_chain_flat_yuv_mix_canvas") and callable(ops.chain_flat_yuv_mix_canvas)


def test_bar_pixels_carry_the_lut_and_layer_2_moves_with_the_canvas(orc):
    """the premises of the GPU cases: a bar pixel of the expectation is LUT(black), not black (a kernel that wrote plain black bars under a LUT would fail), and the
    expectation changes when layer 2 is put at another place on the canvas than layer 1 (a kernel that read layer 2 at the canvas's origin would fail)"""
    lut = gamma_lut(orc)
    lut2 = (255 - np.arange(256)).astype(np.uint8)
    c = case(0xCA1, YUV420P, UYVY, 6, 5, ntracks=1, amounts=[128])
    cv = (11, 9, 3, 2)
    args = (orc, c["f1"], c["f2"], c["frames"][0], c["frames2"][0], c["L1"], c["L2"], 6, 5, 0, 0, 128)
    a, b = expected_canvas(*args, lut2, cv), expected_canvas(*args, None, cv)
    assert (b[0, :4] == [0, 0, 0, 255]).all() and (a[0, :4] == [255, 255, 255, 255]).all() and (expected_canvas(*args, lut, cv)[0, :4] == [lut[0]] * 3 + [255]).all()
    l2 = letterboxed(to_rgba(orc, UYVY, c["frames2"][0], 6, 5, 0, c["L2"]), 6, 5, (11, 9, 0, 0))
    pl, st = c["frames"][0]
    moved = oracle_flat(orc, pl[0], pl[1], pl[2], st, 6, 5, 0, 0, 0, 2, 0, l2, 128, None, cv, RGBA, 0)[0]
    assert (moved != b).any()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(FRAMES)), ids=["%dx%d" % g for g in FRAMES])
def test_mix_canvas_smallest_frames(gpu, orc, k):
    """1. each unit kind at the frame's edge -- row 0, a row pair, the trailing row -- at every offset (bars right of and below the frame too), then on the canvases with
    no bars and with bars on one side only; the pair moves on with every canvas, so all nine are seen on every frame.  Two tracks, amounts 0 and 255"""
    sw, sh = FRAMES[k]
    lut = gamma_lut(orc)
    canvases = [("at (%d, %d)" % o, (sw + o[0] + 3, sh + o[1] + 2, o[0], o[1])) for o in OFFSETS] + [("at (%d, %d), tight" % o, (sw + o[0], sh + o[1], o[0], o[1])) for o in OFFSETS[1:]]
    for j, (what, cv) in enumerate(canvases + extents(sw, sh)):
        f1, f2 = PAIRS[(j + 2 * k) % len(PAIRS)]
        f1, f2 = packed_as(f1, j & 1), packed_as(f2, j & 2)
        rng = np.random.default_rng([0xC51, k, j])
        c = case([0xC52, k, j], f1, f2, sw, sh, ntracks=2, L1=layer(wt=j & 1, q=1 + j % 3, fix=j & 1, pad=(4 * (j & 1), 1, 3), tight=bool(j & 2)),
                 L2=layer(wt=1 - (j & 1), q=3 - j % 3, fix=1 - (j & 1), pad=(4 - 4 * (j & 1), 3, 1), tight=not j & 2), amounts=distinct_amounts(rng, 2))
        run(gpu, orc, c, cv, lut=[None, lut, INVERTED][j % 3], order=(j >> 1) & 1, swap=j & 1, pad=4 * (j % 3))


ALL_PAIRS = PAIRS + [(YUYV, UYVY), (YUV420P, YUYV)]


@pytest.mark.gpu
@pytest.mark.parametrize("pair", ALL_PAIRS, ids=[pair_id(p) for p in ALL_PAIRS])
def test_mix_canvas_format_pairs(gpu, orc, pair):
    """2. all nine pairs of the three walks, and YUYV once on either layer: with and without the LUT, with and without swap_rb, the two layers under different table
    sets (so layer 2's own staged tables are used), on an even and an odd offs_x"""
    f1, f2 = pair
    lut = gamma_lut(orc)
    for j, (with_lut, swap) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        wt1 = j & 1
        L1 = layer(wt=wt1, q=1 + j % 3, fix=j & 1, pad=(4, 3, 1), tight=bool(j & 1), yvu=bool(j & 2))
        L2 = layer(wt=1 - wt1 if (packed(f1) or packed(f2)) else (wt1 + 1 + j % 3) & 3, q=3 - j % 3, fix=1 - (j & 1), pad=(0, 1, 5), tight=not j & 1, yvu=not j & 2)
        assert L1["wt"] != L2["wt"]
        rng = np.random.default_rng([0xC53, f1, f2, j])
        c = case([0xC54, f1, f2, j], f1, f2, 36, 21, ntracks=2, L1=L1, L2=L2, amounts=distinct_amounts(rng, 2) if j == 0 else None)
        run(gpu, orc, c, (36 + 9, 21 + 6, 4 + (j & 1), 3), lut=lut if with_lut else None, order=(j >> 1) & 1, swap=swap)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [(YUV420P, YUV420P), (YUV422P, UYVY), (UYVY, YUV422P)], ids=pair_id)
def test_mix_canvas_second_column_of_workgroups(gpu, orc, pair):
    """3. a frame 516 wide: chroma width 258, so the second column of workgroups has a tail of 2 lanes; 3 high inside a 520 x 5 canvas"""
    c = case([0xC55, pair[0], pair[1]], pair[0], pair[1], 516, 3, ntracks=1, L1=layer(pad=(4, 1, 3)), L2=layer(wt=1, pad=(0, 3, 1)))
    run(gpu, orc, c, (520, 5, 3, 1), lut=gamma_lut(orc), swap=1)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [(YUV420P, YUV422P), (UYVY, YUV420P)], ids=pair_id)
def test_mix_canvas_run_of_units(gpu, orc, pair):
    """4. a frame 2 wide and 4101 high: 2051 units, more than a launch has workgroup rows, so each workgroup walks a run of units; inside a 4 x 4103 canvas"""
    c = case([0xC56, pair[0], pair[1]], pair[0], pair[1], 2, 4101, ntracks=1, L1=layer(pad=(4, 1, 1)), L2=layer(wt=1))
    run(gpu, orc, c, (4, 4103, 1, 1), lut=gamma_lut(orc))


@pytest.mark.gpu
def test_mix_canvas_bar_strides(gpu, orc):
    """5. a 600 x 300 canvas around a 2 x 2 frame: 179,996 bar pixels for 64 bar workgroups, each walking eleven strides of its loop.  Under a LUT that does not keep
    black, so a bar pixel that skipped it shows"""
    rng = np.random.default_rng(0xC57)
    c = case(0xC58, YUV422P, YUV420P, 2, 2, ntracks=2, L2=layer(wt=1), amounts=distinct_amounts(rng, 2))
    run(gpu, orc, c, (600, 300, 301, 149), lut=INVERTED, swap=1, order=1)


@pytest.mark.gpu
@pytest.mark.parametrize("ntracks", [1, 32, 33, 64])
def test_mix_canvas_tracks(gpu, orc, ntracks):
    """6. one launch up to 32 tracks, two from 33 on; every track has its own frames, amount (0 and 255 among them) and destination, in shuffled buffers"""
    rng = np.random.default_rng([0xC59, ntracks])
    f1, f2 = [(UYVY, YUV420P), (YUV420P, YUV420P), (YUV422P, YUYV), (YUV420P, YUV422P)][[1, 32, 33, 64].index(ntracks)]
    c = case([0xC5A, ntracks], f1, f2, 6, 5, ntracks=ntracks, L1=layer(pad=(4, 1, 3)), L2=layer(wt=1, pad=(0, 3, 1)), amounts=distinct_amounts(rng, ntracks))
    run(gpu, orc, c, (10, 8, 1, 2), lut=gamma_lut(orc), swap=ntracks & 1)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [(YUV420P, UYVY), (YUV422P, YUV420P)], ids=pair_id)
def test_mix_canvas_without_a_canvas_is_the_mix_form(gpu, orc, pair):
    """7. canvas == NULL: the bytes of lgpu_chain_flat_yuv_mix without a sink -- the oracle's, and the device's own from that entry point"""
    import torch
    ops = gpu
    f1, f2 = pair
    sw, sh = 36, 21
    c = case([0xC5B, f1, f2], f1, f2, sw, sh, ntracks=2, L1=layer(pad=(4, 1, 3)), L2=layer(wt=1, pad=(0, 3, 1)))
    lut = gamma_lut(orc)
    stride = sw * 4 + 8
    fill = np.random.default_rng(0xC5C).integers(0, 256, (2, sh + GUARD, stride), dtype=np.uint8)
    d1, d2 = [[up(p) for p in fr[0]] for fr in c["frames"]], [[up(p) for p in fr[0]] for fr in c["frames2"]]
    prm = ops.chain_params(sw, sh, 0, sw, sh, 0, stride, swap_rb=1, interp=PIXBUF, bf=0, lut=lut)
    src, src2 = source_of(ops, f1, c["frames"][0], c["L1"], 0), source_of(ops, f2, c["frames2"][0], c["L2"], 1)
    got = []
    for call in (ops.chain_flat_yuv_mix_canvas, ops.chain_flat_yuv_mix):
        dd = [dev_at(fill[i], 0) for i in range(2)]
        trk = ops.chain_yuv_mix_tracks([d[0] for d in d1], None if packed(f1) else [d[1] for d in d1], None if packed(f1) else [d[2] for d in d1],
                                       [d[0] for d in d2], None if packed(f2) else [d[1] for d in d2], None if packed(f2) else [d[2] for d in d2], [[d] for d in dd])
        call(prm, src, src2, trk, c["amounts"])
        torch.cuda.synchronize()
        got.append([host(d) for d in dd])
    for i in range(2):
        want = expected_mix(orc, f1, f2, c["frames"][i], c["frames2"][i], c["L1"], c["L2"], sw, sh, 0, 1, c["amounts"][i], lut, RGBA, 0)[0]
        assert (got[0][i] == got[1][i]).all()
        assert (got[0][i][:sh, :sw * 4] == want).all() and (got[0][i][:sh, sw * 4:] == fill[i][:sh, sw * 4:]).all() and (got[0][i][sh:] == fill[i][sh:]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [(YUV420P, YUV420P), (UYVY, YUV422P), (YUV422P, YUYV)], ids=pair_id)
def test_mix_canvas_refusals(gpu, pair):
    """8. LGPU_E_BADARG and LGPU_E_UNSUPPORTED, one call each: the code is compared and the destination's fill is still whole afterwards; the same call inside the form
    then runs and writes the canvas only"""
    import torch
    from lives_amd import lib
    ops = gpu
    f1, f2 = pair
    w, h = 64, 36
    CW, CH = w + 16, h + 8

    def planes(f, y, u, v):
        if packed(f):
            return [torch.full((h, w * 2), y, dtype=torch.uint8, device="cuda"), None, None], (w * 2, 0, 0)
        ch = (h + 1) // 2 if f == YUV420P else h
        return [torch.full((h, w), y, dtype=torch.uint8, device="cuda")] + [torch.full((ch, w // 2), c, dtype=torch.uint8, device="cuda") for c in (u, v)], (w, w // 2, w // 2)
    (A, full1), (B, full2) = planes(f1, 0, 0, 0), planes(f2, 200, 90, 160)
    orow0 = CW * 4 + 32
    D = torch.full((CH + 8, orow0), 0x5C, dtype=torch.uint8, device="cuda")
    csize = lambda pl: 0 if pl[1] is None else pl[1].numel()
    ptr = lambda t: None if t is None else t.data_ptr()

    def call(canvas=(CW, CH, 5, 3), sw_=w, sh_=h, dw_=None, dh_=None, interp=PIXBUF, blur=0, amounts=(9,), ntracks=1, null=None, strides=full1, strides2=full2, usz=None,
             usz2=None, order=0, order2=None, swap=0, wt_src=0, wt_src2=0, q=2, q2=2, flags2=0, orow=orow0, dst_off=0, in_place=None, in_fmt=f1, in_fmt2=f2, off2=0, no_src2=False):
        dw_, dh_ = sw_ if dw_ is None else dw_, sh_ if dh_ is None else dh_
        prm = ops.chain_params(sw_, sh_, 0, dw_, dh_, 0, orow, swap_rb=swap, interp=interp, do_blur=blur, bf=0)
        src = ops.yuv_layer_source(in_fmt, strides, csize(A) if usz is None else usz, csize(A), out_order=order, which_tables=wt_src, pb_quality=q)
        src2 = ops.yuv_layer_source(in_fmt2, strides2, csize(B) if usz2 is None else usz2, csize(B), out_order=(order ^ swap) if order2 is None else order2,
                                    which_tables=wt_src2, pb_quality=q2, flags=flags2)
        m = max(ntracks, 1)
        trk = (lib.ChainYuvMixTrack * m)()
        for t in trk:
            t.y_d, t.u_d, t.v_d = ptr(A[0]), ptr(A[1]), ptr(A[2])
            t.y2_d, t.u2_d, t.v2_d = ptr(B[0]) + off2, ptr(B[1]), ptr(B[2])
            t.dst_d[0] = D.data_ptr() + dst_off
        if null == "dst":
            trk[0].dst_d[0] = None
        elif null is not None:
            setattr(trk[0], null, None)
        if in_place is not None:
            trk[0].dst_d[0] = (A + B)[in_place].data_ptr()
        if ntracks < 1:
            trk = (lib.ChainYuvMixTrack * 0)()
        if no_src2:
            cv = lib.Canvas(*canvas)
            return lib.load().lgpu_chain_flat_yuv_mix_canvas(ctypes.byref(prm), ctypes.byref(src), None, ctypes.byref(cv), trk, len(trk), (ctypes.c_uint8 * m)(*(list(amounts) * m)),
                                                             ops.stream_ptr())
        return ops.chain_flat_yuv_mix_canvas(prm, src, src2, trk, list(amounts) * m if amounts is not None else None, canvas=canvas, check=False)

    badarg = {
        "canvas narrower than the frame": dict(canvas=(w - 2, CH, 0, 0)),
        "canvas lower than the frame": dict(canvas=(CW, h - 1, 0, 0)),
        "frame past the canvas's right edge": dict(canvas=(CW, CH, 17, 0)),
        "frame past the canvas's lower edge": dict(canvas=(CW, CH, 0, 9)),
        "negative offs_x": dict(canvas=(CW, CH, -1, 0)),
        "negative offs_y": dict(canvas=(CW, CH, 0, -1)),
        "destination stride below the canvas row": dict(orow=CW * 4 - 4),
        "destination stride of the frame's row, not the canvas's": dict(orow=w * 4),
        "destination stride not a multiple of 4": dict(orow=orow0 + 2),
        "destination not 4-byte aligned": dict(dst_off=2),
        "null destination": dict(null="dst"),
        "destination is layer 1's frame / luma plane": dict(in_place=0),
        "destination is layer 2's frame / luma plane": dict(in_place=3),
        "no PIXBUF": dict(interp=3),
        "NOBLEND": dict(interp=PIXBUF | NOBLEND),
        "null amounts": dict(amounts=None),
        "no tracks": dict(ntracks=0),
        "65 tracks": dict(ntracks=65),
        "null src2": dict(no_src2=True),
        "in_fmt 1": dict(in_fmt=1),
        "src2 in_fmt 6": dict(in_fmt2=6),
        "null layer-1 frame / luma plane": dict(null="y_d"),
        "null layer-2 frame / luma plane": dict(null="y2_d"),
        "src2 out_order against the chain's (no swap)": dict(order=1, swap=0, order2=0),
        "src2 out_order against the chain's (swap)": dict(order=1, swap=1, order2=1),
        "source which_tables 4": dict(wt_src=4),
        "src2 which_tables -1": dict(wt_src2=-1),
        "pb_quality 0": dict(q=0),
        "src2 pb_quality 4": dict(q2=4),
        "src2 unknown flag": dict(flags2=2),
        "first stride below the row": dict(strides=(full1[0] - 4,) + full1[1:]),
        "src2 first stride below the row": dict(strides2=(full2[0] - 4,) + full2[1:]),
        "odd sw": dict(sw_=w - 1),
        "sh 0": dict(sh_=0),
    }
    unsupported = {
        "2:1": dict(dw_=w // 2, dh_=h // 2),
        "another width": dict(dw_=w + 2),
        "another height": dict(dh_=h - 1),
        "gaussian": dict(blur=1),
        "first plane of 2 GiB": dict(strides=(1 << 26, full1[1], full1[2])),
        "layer-2 first plane of 2 GiB": dict(strides2=(1 << 26, full2[1], full2[2])),
        "canvas-sized destination of 2 GiB": dict(orow=1 << 26),
    }
    if packed(f1):
        badarg["BT.709 tables with a packed layer 1"] = dict(wt_src=2)
    else:
        badarg.update({"null U plane": dict(null="u_d"), "U plane one byte short": dict(usz=csize(A) - 1), "destination is layer 1's V plane": dict(in_place=2)})
        unsupported["U plane of 2 GiB"] = dict(usz=1 << 31)
    if packed(f2):
        badarg["BT.709 tables with a packed layer 2"] = dict(wt_src2=3)
        unsupported.update({"packed layer-2 rowstride % 4 == 2": dict(strides2=(w * 2 + 2, 0, 0)), "packed layer-2 plane at 2 mod 4": dict(off2=2)})
    else:
        badarg.update({"null layer-2 V plane": dict(null="v2_d"), "layer-2 U plane one byte short": dict(usz2=csize(B) - 1), "destination is layer 2's U plane": dict(in_place=4)})
        unsupported["layer-2 U plane of 2 GiB"] = dict(usz2=1 << 31)
    for want, table in ((E_BADARG, badarg), (E_UNSUPPORTED, unsupported)):
        for what, kw in table.items():
            rc = call(**kw)
            torch.cuda.synchronize()
            assert rc == want, "%s (%s): %d, expected %d (%s)" % (what, kw, rc, want, lib.load().lgpu_last_error())
            assert bool((D == 0x5C).all()), "%s: the destination was written" % what
    # ... and the same call inside the form runs: the canvas, bars included, and nothing else
    assert call(amounts=(128,)) == 0
    torch.cuda.synchronize()
    assert bool((D[:CH, 3:CW * 4:4] == 255).all()) and bool((D[CH:] == 0x5C).all()) and bool((D[:, CW * 4:] == 0x5C).all())          # every pixel's alpha
    assert call(canvas=(CW, CH, 16, 8)) == 0 and call(canvas=(w, h, 0, 0)) == 0          # the frame in the canvas's corner; a canvas the frame fills
    torch.cuda.synchronize()
