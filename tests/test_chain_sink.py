"""lgpu_chain_to_yuv: the 2:1 chain that ENDS at a YUV sink ([R <-> B] -> the exact 2:1 scaler -> [chroma blend] -> [gamma LUT] -> K4's conversion to UYVY / YUYV /
YUV420P, one launch, no RGBA frame) against the oracle's composition tests.chain_ref.oracle_chain_rgba -> orc_rgb_to_yuv(.., in_order, 1, .., out_fmt, 0,
which_tables); at size against the two-launch form lgpu_chain_amounts + lgpu_rgb_to_yuv_batch; and its refusals.  Bit-exact: every byte of every plane, and every
byte of the planes' row padding and guard rows."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.chain_ref import distinct_amounts, oracle_chain_rgba
from tests.util import align, dev, host

pytestmark = pytest.mark.gpu
P = po.P
PIXBUF, NOBLEND = 0x100, 0x400
E_BADARG, E_UNSUPPORTED = -2, -3
UYVY, YUYV, YUV420P = 2, 3, 4
GUARD = 2


def gamma_lut(orc):
    lut = np.zeros(256, np.uint8)
    assert orc.orc_gamma_lut8(1.0, po.GAMMA_SRGB, po.GAMMA_LINEAR, 1.4, P(lut)) == 1
    return lut


def plane_dims(fmt, dw, dh):
    """(bytes per row, rows) of the sink's planes"""
    return [(dw * 2, dh)] if fmt in (UYVY, YUYV) else [(dw, dh), (dw >> 1, dh >> 1), (dw >> 1, dh >> 1)]


def oracle_sink(orc, rgba, dw, dh, fmt, in_order, wt):
    """K4 on the chain's RGBA result, into compact planes (the reference's 4:2:0 and UYVY row arithmetic exists on compact rows only)"""
    want, _ = po.k4_out_planes(0, dw, dh, fmt, 0)
    wp, ws = po.planes_args(want)
    assert orc.orc_rgb_to_yuv(P(rgba), rgba.strides[0], dw, dh, in_order, 1, ctypes.addressof(wp), ctypes.addressof(ws), fmt, 0, wt) == 0
    return want


def random_source(rng, sw, sh):
    src = rng.integers(0, 256, (sh, align(sw * 4, 16) + 16), dtype=np.uint8)
    al = src[:, 3:sw * 4:4]
    al[rng.random(al.shape) < 0.5] = 255          # half of the source opaque, the rest translucent: the scaler weights colours by alpha
    return src


def run(gpu, orc, rng, sw, sh, fmt, ntracks=1, interp=3, blend=True, lut=None, wt=0, in_order=0, swap=0, yvu=False, pads=(8, 4, 12), srcs=None):
    """one launch of ntracks tracks that all differ; the device buffers are allocated in a shuffled order and handed over in another (slot order != frame order);
    Y, U and V planes have different paddings; every plane is compared whole: frame bytes against the oracle, row padding and guard rows against their fill.
    Returns the expected planes of every track."""
    ops = gpu
    dw, dh = sw // 2, sh // 2
    dims = plane_dims(fmt, dw, dh)
    strides = [align(b + pads[k], 8 if k == 0 else 4) for k, (b, _) in enumerate(dims)]
    irow2 = align(dw * 4, 8) + 24
    srcs = srcs if srcs is not None else [random_source(rng, sw, sh) for _ in range(ntracks)]
    l2s = None
    if blend:
        l2s = [rng.integers(0, 256, (dh, irow2), dtype=np.uint8) for _ in range(ntracks)]
        for a in l2s:
            al = a[:, 3:dw * 4:4]
            al[rng.random(al.shape) < 0.5] = 255
    amounts = distinct_amounts(rng, ntracks)
    fills = [[rng.integers(0, 256, (r + GUARD, strides[k]), dtype=np.uint8) for k, (_, r) in enumerate(dims)] for _ in range(ntracks)]
    d_src, d_l2, d_pl = [None] * ntracks, [None] * ntracks, [None] * ntracks
    for i in rng.permutation(ntracks):
        d_pl[i] = [dev(f) for f in fills[i]]
        d_src[i] = dev(srcs[i])
        d_l2[i] = dev(l2s[i]) if blend else None
    order = [int(k) for k in rng.permutation(ntracks)]
    # YVU420P: the layer's second plane is V -- the chain is handed the planes in Y, U, V order, so buffer 2 takes U and buffer 1 takes V
    sel = [0, 2, 1] if (yvu and fmt == YUV420P) else list(range(len(dims)))
    prm = ops.chain_params(sw, sh, srcs[0].strides[0], dw, dh, irow2, 0, swap_rb=swap, interp=interp | PIXBUF | (0 if blend else NOBLEND), bf=0, lut=lut)
    sink = ops.chain_sink(fmt, [strides[j] for j in sel], which_tables=wt, in_order=in_order)
    trk = ops.chain_sink_tracks([d_src[k] for k in order], [d_l2[k] for k in order] if blend else None, [[d_pl[k][j] for j in sel] for k in order])
    ops.chain_to_yuv(prm, sink, trk, [amounts[k] for k in order] if blend else None)
    wants = []
    for i in range(ntracks):
        rgba = oracle_chain_rgba(orc, srcs[i], sw, sh, dw, dh, interp, swap, l2s[i] if blend else None, amounts[i] if blend else 0, lut)
        want = oracle_sink(orc, rgba, dw, dh, fmt, in_order, wt)
        wants.append(want)
        for p, j in enumerate(sel):              # p: the conversion's plane (Y, U, V); j: the buffer it was handed
            b, r = dims[p]
            got = host(d_pl[i][j])
            bad = got[:r, :b] != want[p][:r, :b]
            assert not bad.any(), "track %d plane %d: %d bytes differ from the oracle, first at %s" % (i, p, int(bad.sum()), np.argwhere(bad)[0].tolist())
            assert (got[:r, b:] == fills[i][j][:r, b:]).all(), "track %d plane %d: row padding was written" % (i, p)
            assert (got[r:] == fills[i][j][r:]).all(), "track %d plane %d: guard rows were written" % (i, p)
    return wants


GEOM = [(256, 144), (264, 100), (520, 292), (8, 4), (16, 4), (16, 12)]       # dw % 8 == 0 / 4; more than one strip of 128 columns; one chroma row (the "last row alone" rule only)
BIG, SMALL = GEOM[:3], GEOM[3:]


def stage_geometries(interp, blend, with_lut, fmt):
    """the two geometries of a stage-matrix case, chosen so that EVERY format and every (filter, blend) pair of it -- every kernel instantiation -- meets 520x292 -> 260x146
    (three strips, dw % 8 == 4: a half-filled last quad, 25 bands: odd bands walk upwards) and 8x4 -> 4x2 (a lone half quad, no inner row pair), and the other four
    geometries of the list are spread over the rest"""
    ib = (interp == 2) * 2 + (not blend)
    if with_lut:
        return [BIG[2], SMALL[1 + (ib + fmt) % 2]]
    return [BIG[(ib + fmt) % 2], SMALL[0]]


@pytest.mark.parametrize("interp", [3, 2], ids=["hyper", "bilinear"])
@pytest.mark.parametrize("blend", [True, False], ids=["blend", "noblend"])
@pytest.mark.parametrize("with_lut", [True, False], ids=["lut", "nolut"])
@pytest.mark.parametrize("fmt", [UYVY, YUYV, YUV420P], ids=["uyvy", "yuyv", "yuv420p"])
def test_chain_sink_stages(gpu, orc, interp, blend, with_lut, fmt):
    """every stage combination to every sink format, each on two geometries (stage_geometries) and with both settings of swap_rb on each, in_order and which_tables
    drawn per run, against the oracle"""
    case = ((interp == 2) * 4 + (not blend) * 2 + (not with_lut)) * 3 + (fmt - 2)
    rng = np.random.default_rng(0x51C0 + case)
    lut = gamma_lut(orc) if with_lut else None
    for i, (sw, sh) in enumerate(stage_geometries(interp, blend, with_lut, fmt)):
        for swap in (0, 1):
            wt = int(rng.integers(0, 4)) if fmt == YUV420P else int(rng.integers(0, 2))
            run(gpu, orc, rng, sw, sh, fmt, ntracks=2, interp=interp, blend=blend, lut=lut, wt=wt, in_order=int(rng.integers(0, 2)), swap=swap,
                yvu=bool(i), pads=(8 * i, 4 + i, 12 - 3 * i))


def test_stage_matrix_covers_every_geometry_for_every_format():
    """the choice above, checked: per format and (filter, blend) pair the multi-strip frame and 4x2 are met, and per format all six geometries of the list"""
    for fmt in (UYVY, YUYV, YUV420P):
        seen_fmt = set()
        for interp in (3, 2):
            for blend in (True, False):
                seen = set()
                for with_lut in (True, False):
                    seen.update(stage_geometries(interp, blend, with_lut, fmt))
                assert (520, 292) in seen and (8, 4) in seen, (fmt, interp, blend, seen)
                seen_fmt |= seen
        assert seen_fmt == set(GEOM), (fmt, seen_fmt)


def corner_source(dw, dh, colour_of):
    """an opaque source whose every 2 x 2 block is one pure 0 / 255 colour: the BILINEAR 2:1 reduction (taps 2X, 2X + 1 only) gives destination pixel (x, y) exactly
    the colour colour_of(x, y) = (r, g, b)"""
    src = np.zeros((2 * dh, 2 * dw * 4), np.uint8)
    px = src.reshape(2 * dh, 2 * dw, 4)
    px[..., 3] = 255
    for y in range(dh):
        for x in range(dw):
            px[2 * y:2 * y + 2, 2 * x:2 * x + 2, :3] = colour_of(x, y)
    return src


def corner(i):
    return (255 * (i & 1), 255 * ((i >> 1) & 1), 255 * ((i >> 2) & 1))


@pytest.mark.parametrize("fmt,wt", [(YUV420P, 0), (YUV420P, 1), (YUV420P, 2), (YUV420P, 3), (UYVY, 0), (UYVY, 1), (YUYV, 0), (YUYV, 1)])
def test_chain_sink_clamp_bounds(gpu, orc, fmt, wt):
    """the eight corner colours on opaque 2:1-proof blocks, no blend, no LUT: Y 16 / 235 and chroma 16 / 240 with clamped tables, 0 / 255 with unclamped ones -- every
    clamp bound is reached (asserted on the EXPECTED planes), in both byte orders"""
    rng = np.random.default_rng(0xC1A + fmt * 4 + wt)
    dw, dh = 32, 16
    # every colour on even and on odd columns and rows; the last row (the 4:2:0 walk's unaveraged chroma row) has them all too
    src = corner_source(dw, dh, lambda x, y: corner((x + 3 * y + (x >> 3)) & 7))
    for in_order in (0, 1):
        want = run(gpu, orc, rng, 2 * dw, 2 * dh, fmt, interp=2, blend=False, wt=wt, in_order=in_order, srcs=[src])[0]
        lo, hy, hc = (0, 255, 255) if wt & 1 else (16, 235, 240)
        if fmt == YUV420P:
            luma, chroma = want[0], np.concatenate([want[1][-1], want[2][-1]])        # the last chroma row is row dh - 1's alone: no average between it and the clamp
        elif fmt == UYVY:
            luma, chroma = want[0][:, 1::2], want[0][:, 0::2]
        else:
            luma, chroma = want[0][:, 0::2], want[0][:, 1::2]
        assert int(luma.min()) == lo and int(luma.max()) == hy, (int(luma.min()), int(luma.max()))
        if fmt == YUYV and wt & 1:
            assert int(chroma.min()) == 0            # rgb2yuyv has no upper chroma clamp: raw 256 is stored as byte 0 (next test)
        else:
            assert int(chroma.min()) == lo and int(chroma.max()) == hc, (int(chroma.min()), int(chroma.max()))


def test_chain_sink_yuyv_lost_upper_clamp(gpu, orc):
    """unclamped tables, pure blue on even and pure red on odd destination columns: U raw 256 / V raw 256, which rgb2yuyv (no `else`: only the lower clamp survives)
    stores as byte 0 where rgb2uyvy stores 255.  The expectation itself is asserted to show the quirk, so the comparison cannot pass vacuously."""
    rng = np.random.default_rng(0x10C)
    dw, dh = 24, 6
    src = corner_source(dw, dh, lambda x, y: (0, 0, 255) if not (x & 1) else (255, 0, 0))
    w_yuyv = run(gpu, orc, rng, 2 * dw, 2 * dh, YUYV, interp=2, blend=False, wt=1, srcs=[src])[0][0]
    w_uyvy = run(gpu, orc, rng, 2 * dw, 2 * dh, UYVY, interp=2, blend=False, wt=1, srcs=[src])[0][0]
    assert (w_yuyv[:, 1::2] == 0).all() and (w_uyvy[:, 0::2] == 255).all()
    assert (w_yuyv[:, 0::2] == w_uyvy[:, 1::2]).all()          # luma agrees
    # with clamped tables no colour exceeds 240 and the two formats agree
    c_yuyv = run(gpu, orc, rng, 2 * dw, 2 * dh, YUYV, interp=2, blend=False, wt=0, srcs=[src])[0][0]
    c_uyvy = run(gpu, orc, rng, 2 * dw, 2 * dh, UYVY, interp=2, blend=False, wt=0, srcs=[src])[0][0]
    assert (c_yuyv[:, 1::2] == c_uyvy[:, 0::2]).all()


@pytest.mark.parametrize("th", [1, 2, 5, 7])
@pytest.mark.parametrize("sw,sh", [(512, 200), (248, 1000)])
def test_chain_sink_band_seams_at_forced_heights(gpu, orc, tune, sw, sh, th):
    """the 4:2:0 form with bands of (about) th rows requested: its band boundaries lie at odd rows whatever is asked for, and the bytes do not depend on it"""
    tune("PBH_TH", th)
    rng = np.random.default_rng(0xBA5D + sw + th)
    run(gpu, orc, rng, sw, sh, YUV420P, ntracks=2, interp=3, blend=True, lut=gamma_lut(orc), wt=th & 3, in_order=th & 1, swap=1, pads=(0, 8, 4))


@pytest.mark.parametrize("ntracks", [1, 7, 16, 17, 64])
def test_chain_sink_tracks(gpu, orc, ntracks):
    """1 .. 64 tracks in one launch with distinct amounts and shuffled buffers, to every format; YVU by swapped planes; guard rows and row padding of all planes"""
    rng = np.random.default_rng(0x7AC + ntracks)
    lut = gamma_lut(orc)
    run(gpu, orc, rng, 264, 100, YUV420P, ntracks=ntracks, blend=True, lut=lut, wt=2, in_order=1, swap=1, yvu=True, pads=(4, 8, 0))
    run(gpu, orc, rng, 264, 100, UYVY, ntracks=ntracks, blend=True, lut=lut, wt=0, pads=(12, 0, 0))
    run(gpu, orc, rng, 264, 100, YUYV, ntracks=ntracks, interp=2, blend=True, wt=1, in_order=1, pads=(0, 0, 0))


@pytest.mark.parametrize("fmt", [YUV420P, UYVY], ids=["yuv420p", "uyvy"])
def test_chain_sink_at_size_matches_two_launches(gpu, orc, fmt):
    """16 x 3840x2160 -> 1920x1080 with blend and gamma: byte-identical to lgpu_chain_amounts + lgpu_rgb_to_yuv_batch on the same inputs; track 0 against the
    oracle as well"""
    import torch
    ops = gpu
    rng = np.random.default_rng(0x51 + fmt)
    sw, sh, dw, dh, n = 3840, 2160, 1920, 1080, 16
    lut = gamma_lut(orc)
    g = torch.Generator(device="cuda")
    g.manual_seed(4321 + fmt)
    S = [torch.randint(0, 256, (sh, sw * 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    for s in S:
        s[::2, 3::4] = 255        # opaque and translucent source pixels
    L2 = [torch.randint(0, 256, (dh, dw * 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    amounts = [int(x) for x in rng.integers(0, 256, n)]
    dims = plane_dims(fmt, dw, dh)
    fused = [[torch.full((r, b), 0x5C, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
    two = [[torch.full((r, b), 0xC5, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
    prm = ops.chain_params(sw, sh, sw * 4, dw, dh, dw * 4, dw * 4, swap_rb=1, interp=3 | PIXBUF, bf=0, lut=lut)
    ops.chain_to_yuv(prm, ops.chain_sink(fmt, [b for (b, _) in dims], which_tables=0, in_order=0), ops.chain_sink_tracks(S, L2, fused), amounts)
    rgba = [torch.zeros((dh, dw * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    ops.chain_amounts(prm, ops.chain_tracks(S, L2, rgba), amounts)
    ops.rgb_to_yuv_batch(rgba, two, dw, dh, 0, 1, fmt, 0, 0)
    torch.cuda.synchronize()
    for i in range(n):
        for p in range(len(dims)):
            assert torch.equal(fused[i][p], two[i][p]), "track %d plane %d: %d bytes differ from the two-launch form" % (i, p, int((fused[i][p] != two[i][p]).sum()))
    want_rgba = oracle_chain_rgba(orc, host(S[0]), sw, sh, dw, dh, 3, 1, host(L2[0]), amounts[0], lut)
    want = oracle_sink(orc, want_rgba, dw, dh, fmt, 0, 0)
    for p in range(len(dims)):
        assert (host(fused[0][p]) == want[p]).all(), "plane %d differs from the oracle" % p


def test_chain_sink_refusals(gpu):
    """bad arguments: LGPU_E_BADARG; shapes off the one-launch form: LGPU_E_UNSUPPORTED; nothing is written in either case; the same call inside the form runs"""
    import torch
    from lives_amd import lib
    ops = gpu
    sw, sh, dw, dh = 256, 144, 128, 72
    S = torch.zeros((sh + 2, sw * 4 + 64), dtype=torch.uint8, device="cuda")
    L2 = torch.zeros((dh + 8, dw * 4 + 64), dtype=torch.uint8, device="cuda")
    D = [torch.full((dh + 8, dw * 2 + 64), 0x5C, dtype=torch.uint8, device="cuda") for _ in range(3)]

    def call(fmt=YUV420P, sw_=sw, sh_=sh, dw_=dw, dh_=dh, interp=3 | PIXBUF, blur=0, amounts=(9,), ntracks=1, planes=True, wt=0, in_order=0, orow=None, irow=sw * 4 + 64,
             src_off=0, dst_off=0):
        prm = ops.chain_params(sw_, sh_, irow, dw_, dh_, dw * 4 + 64, 0, swap_rb=0, interp=interp, do_blur=blur, bf=0)
        sink = ops.chain_sink(fmt, orow if orow is not None else [dw * 2 + 64] * 3, which_tables=wt, in_order=in_order)
        m = max(ntracks, 1)
        trk = ops.chain_sink_tracks([S] * m, [L2] * m, [D] * m)
        for t in trk:
            t.src_d += src_off
            t.dst_d[0] += dst_off
        if not planes:
            trk[0].dst_d[2] = None
        if ntracks < 1:
            trk = (lib.ChainSinkTrack * 0)()
        am = list(amounts) * m if amounts is not None else None
        return ops.chain_to_yuv(prm, sink, trk, am, check=False)

    badarg = {
        "no PIXBUF": dict(interp=3),
        "null amounts with a blend": dict(amounts=None),
        "no tracks": dict(ntracks=0),
        "65 tracks": dict(ntracks=65),
        "null plane": dict(planes=False),
        "out_fmt 1": dict(fmt=1),
        "out_fmt 6": dict(fmt=6),
        "in_order 2": dict(in_order=2),
        "BT.709 with UYVY": dict(fmt=UYVY, wt=2),
        "BT.709 with YUYV": dict(fmt=YUYV, wt=3),
        "odd dw": dict(sw_=254, dw_=127),
        "luma stride below the row": dict(orow=[dw - 8, dw, dw]),
        "chroma stride below the row": dict(orow=[dw, dw // 2 - 4, dw]),
        "packed stride below the row": dict(fmt=UYVY, orow=[dw * 2 - 8, 0, 0]),
        "source stride below the row": dict(irow=sw * 4 - 16),
    }
    unsupported = {
        "not 2:1": dict(sw_=sw - 8),
        "dw % 4 == 2": dict(sw_=252, dw_=126),
        "odd dh with 4:2:0": dict(sh_=142, dh_=71),
        "gaussian": dict(blur=1),
        "nearest": dict(interp=0 | PIXBUF),
        "YUV422P": dict(fmt=5),
        "luma rowstride % 8 != 0": dict(orow=[dw + 4, dw, dw]),
        "chroma rowstride % 4 != 0": dict(orow=[dw + 8, dw // 2 + 2, dw]),
        "packed rowstride % 8 != 0": dict(fmt=YUYV, orow=[dw * 2 + 4, 0, 0]),
        "sink plane not 16-byte aligned": dict(dst_off=8),
        "source not 16-byte aligned": dict(src_off=4),
    }
    for what, kw in list(badarg.items()) + list(unsupported.items()):
        want = E_UNSUPPORTED if what in unsupported else E_BADARG
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc == want, "%s: %d, expected %d (%s)" % (what, rc, want, lib.load().lgpu_last_error())
        assert all(bool((d == 0x5C).all()) for d in D), "%s: a sink plane was written" % what
    assert call(sh_=142, dh_=71, fmt=UYVY) == 0      # any dh for the packed formats
    torch.cuda.synchronize()
    assert not bool((D[0][:71, :dw * 2] == 0x5C).all()) and bool((D[1] == 0x5C).all())
    assert call() == 0                                # and the same call inside the form runs
    torch.cuda.synchronize()
    assert not any(bool((d[:dh // 2, :dw // 2] == 0x5C).all()) for d in D)
