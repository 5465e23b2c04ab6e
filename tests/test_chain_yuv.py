"""lgpu_chain_yuv420p: the 2:1 chain that starts at decoded planar 4:2:0 frames (K2's conversion in registers -> the exact 2:1 scaler -> [letterbox] -> [chroma blend]
-> [gamma LUT], one launch) against the oracle's composition of the single stages, orc_yuv420p_to_rgb -> orc_pixbuf_scale -> [orc_letterbox] -> [orc_blend_chroma]
-> [orc_gamma_apply]; at size against the two-launch form lgpu_yuv420p_to_rgb_batch + lgpu_chain_amounts; and its refusals."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests.chain_ref import oracle_chain, planes
from tests.util import align, dev, host

pytestmark = pytest.mark.gpu
P = po.P
PIXBUF, NOBLEND = 0x100, 0x400
E_BADARG, E_UNSUPPORTED = -2, -3


def gamma_lut(orc):
    lut = np.zeros(256, np.uint8)
    assert orc.orc_gamma_lut8(1.0, po.GAMMA_SRGB, po.GAMMA_LINEAR, 1.4, P(lut)) == 1
    return lut


def centred(n, size):
    return (n - size + 1) >> 1        # letterbox_layer's offsets (src/colourspace.c:15522-15523)


def run(gpu, orc, rng, sw, sh, ntracks=1, interp=3, blend=True, lut=None, canvas=False, wt=0, q=2, fix=0, order=0, swap=0, yvu=False,
        pad=(0, 0, 0), tight=False):
    ops = gpu
    dw, dh = sw // 2, sh // 2
    cv = None
    if canvas:
        nw, nh = dw + 12, dh + 10
        cv = (nw, nh, centred(nw, dw), centred(nh, dh))
        assert cv[2] % 2 == 0
    cw, ch = (cv[0], cv[1]) if cv else (dw, dh)
    orow, irow2 = align(cw * 4 + 8, 16), align(cw * 4, 8) + 24
    srcs = [planes(rng, sw, sh, pad, tight) for _ in range(ntracks)]
    l2s = [rng.integers(0, 256, (ch, irow2), dtype=np.uint8) for _ in range(ntracks)] if blend else None
    if blend:
        for a in l2s:
            al = a[:, 3:cw * 4:4]
            al[rng.random(al.shape) < 0.5] = 255
    amounts = [int(x) for x in rng.integers(0, 256, ntracks)] if blend else None
    fill = rng.integers(0, 256, (ch + 1, orow), dtype=np.uint8)
    dsts = [dev(fill) for _ in range(ntracks)]
    # YVU420P: the layer's second plane is V -- the chain is handed the planes in U, V order (swap_chroma_planes)
    d_y = [dev(s[0]) for s in srcs]
    d_p1, d_p2 = [dev(s[1]) for s in srcs], [dev(s[2]) for s in srcs]
    d_u, d_v = (d_p2, d_p1) if yvu else (d_p1, d_p2)
    ys_, us_, vs_ = srcs[0][3]
    stri = (ys_, vs_, us_) if yvu else (ys_, us_, vs_)
    usz, vsz = (srcs[0][2].size, srcs[0][1].size) if yvu else (srcs[0][1].size, srcs[0][2].size)
    prm = ops.chain_params(sw, sh, ys_, dw, dh, irow2, orow, swap_rb=swap, interp=interp | PIXBUF | (0 if blend else NOBLEND), bf=0, lut=lut)
    src = ops.yuv_source(stri, usz, vsz, out_order=order, which_tables=wt, pb_quality=q, flags=fix)
    trk = ops.chain_yuv_tracks(d_y, d_u, d_v, [dev(a) for a in l2s] if blend else None, dsts)
    ops.chain_yuv420p(prm, src, trk, amounts, canvas=cv)
    for t in range(ntracks):
        Y, A1, A2, _ = srcs[t]
        U, V = (A2, A1) if yvu else (A1, A2)
        want = oracle_chain(orc, Y, U, V, stri, sw, sh, interp, order ^ swap, wt, q, fix, l2s[t] if blend else None, amounts[t] if blend else 0, lut, cv)
        got = host(dsts[t])
        bad = got[:ch, :cw * 4] != want
        assert not bad.any(), "track %d: %d bytes differ, first at %s" % (t, int(bad.sum()), np.argwhere(bad)[0].tolist())
        assert (got[:ch, cw * 4:] == fill[:ch, cw * 4:]).all() and (got[ch:] == fill[ch:]).all(), "track %d: bytes outside the frame were written" % t


GEOM = [(256, 144), (260, 146), (132, 76), (264, 100)]       # sw % 8 == 0 / 4, sh % 4 == 0 / 2; two strips of 124 columns from dw = 130 on


@pytest.mark.parametrize("interp", [3, 2], ids=["hyper", "bilinear"])
@pytest.mark.parametrize("blend", [True, False], ids=["blend", "noblend"])
@pytest.mark.parametrize("with_lut", [True, False], ids=["lut", "nolut"])
@pytest.mark.parametrize("canvas", [False, True], ids=["frame", "canvas"])
def test_chain_yuv_stages(gpu, orc, interp, blend, with_lut, canvas):
    """every stage combination, each on two geometries with mixed settings, against the oracle"""
    rng = np.random.default_rng(0x420 + interp * 16 + blend * 8 + with_lut * 4 + canvas * 2)
    lut = gamma_lut(orc) if with_lut else None
    for i, (sw, sh) in enumerate(GEOM[:2] if not canvas else GEOM[2:]):
        run(gpu, orc, rng, sw, sh, ntracks=2, interp=interp, blend=blend, lut=lut, canvas=canvas, wt=int(rng.integers(0, 4)), q=int(rng.integers(1, 4)),
            fix=i & 1, order=int(rng.integers(0, 2)), swap=int(rng.integers(0, 2)), yvu=bool(i & 1), pad=(i * 3, 5, 1), tight=bool(i))


@pytest.mark.parametrize("wt", [0, 1, 2, 3])
@pytest.mark.parametrize("q", [1, 2, 3])
@pytest.mark.parametrize("fix", [0, 1])
def test_chain_yuv_tables_quality_edges(gpu, orc, wt, q, fix):
    """all four table sets (clamped / unclamped, BT.601 / BT.709), pb_quality LOW / MED / HIGH, the trailing row with and without LGPU_YUV_FIX_EDGES"""
    rng = np.random.default_rng(0x1E + wt * 8 + q * 2 + fix)
    run(gpu, orc, rng, 260, 146, interp=3, blend=True, lut=gamma_lut(orc), wt=wt, q=q, fix=fix, pad=(4, 2, 6), tight=True)


@pytest.mark.parametrize("order", [0, 1], ids=["rgba", "bgra"])
@pytest.mark.parametrize("swap", [0, 1], ids=["noswap", "swap"])
@pytest.mark.parametrize("yvu", [False, True], ids=["yuv", "yvu"])
def test_chain_yuv_orders(gpu, orc, order, swap, yvu):
    """RGBA / BGRA output, the chain's R <-> B swap folded in, YUV / YVU plane order (different chroma strides, so a mix-up shows)"""
    rng = np.random.default_rng(0x0D + order * 4 + swap * 2 + yvu)
    run(gpu, orc, rng, 256, 144, interp=3, blend=True, order=order, swap=swap, yvu=yvu, pad=(0, 3, 9))


@pytest.mark.parametrize("pad,tight", [((0, 0, 0), False), ((0, 0, 0), True), ((1, 1, 3), True), ((7, 0, 5), False), ((32, 16, 16), True)],
                         ids=["compact", "compact-tight", "odd-pitches-tight", "odd-luma", "aligned-padding-tight"])
@pytest.mark.parametrize("sw,sh", GEOM)
def test_chain_yuv_pitches(gpu, orc, sw, sh, pad, tight):
    """any luma / chroma pitch, and chroma planes that end exactly at their last sample (the past-the-end read of the last pair clamped)"""
    rng = np.random.default_rng(sw * 7 + sh + sum(pad) + tight)
    run(gpu, orc, rng, sw, sh, interp=3, blend=True, pad=pad, tight=tight)


@pytest.mark.parametrize("ntracks", [1, 7, 16])
def test_chain_yuv_tracks(gpu, orc, ntracks):
    """1, 7 and 16 tracks in one launch, each with its own blend amount"""
    rng = np.random.default_rng(0x7A + ntracks)
    run(gpu, orc, rng, 260, 146, ntracks=ntracks, interp=3, blend=True, lut=gamma_lut(orc), pad=(4, 0, 2))


def test_chain_yuv_small_frames(gpu, orc):
    """the smallest frames: one output row (the first pair and the trailing row only), two, one strip"""
    rng = np.random.default_rng(0x5A11)
    for sw, sh in [(8, 2), (8, 4), (16, 6), (4, 2)]:
        for fix in (0, 1):
            run(gpu, orc, rng, sw, sh, interp=3, blend=True, fix=fix, tight=True)
            run(gpu, orc, rng, sw, sh, interp=2, blend=False, fix=fix)


def test_chain_yuv_at_size_matches_two_launches(gpu, orc):
    """16 x 3840x2160 -> 1920x1080 with blend and gamma: byte-identical to lgpu_yuv420p_to_rgb_batch + lgpu_chain_amounts on the same inputs; track 0 against
    the oracle as well"""
    import torch
    ops = gpu
    rng = np.random.default_rng(0x4C)
    sw, sh, dw, dh, n = 3840, 2160, 1920, 1080, 16
    lut = gamma_lut(orc)
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    Ys = [torch.randint(0, 256, (sh, sw), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    Us = [torch.randint(0, 256, (sh // 2, sw // 2), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    Vs = [torch.randint(0, 256, (sh // 2, sw // 2), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    L2 = [torch.randint(0, 256, (dh, dw * 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    amounts = [int(x) for x in rng.integers(0, 256, n)]
    fused = [torch.zeros((dh, dw * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    two = [torch.zeros((dh, dw * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    prm = ops.chain_params(sw, sh, sw * 4, dw, dh, dw * 4, dw * 4, swap_rb=0, interp=3 | PIXBUF, bf=0, lut=lut)
    ops.chain_yuv420p(prm, ops.yuv_source((sw, sw // 2, sw // 2), Us[0].numel(), Vs[0].numel()), ops.chain_yuv_tracks(Ys, Us, Vs, L2, fused), amounts)
    rgba = [torch.zeros((sh, sw * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    ops.yuv420p_to_rgb_batch([(Ys[i], Us[i], Vs[i], rgba[i]) for i in range(n)], sw, sh)
    ops.chain_amounts(prm, ops.chain_tracks(rgba, L2, two), amounts)
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(fused[i], two[i]), "track %d: %d bytes differ from the two-launch form" % (i, int((fused[i] != two[i]).sum()))
    Y, U, V = host(Ys[0]), host(Us[0]), host(Vs[0])
    want = oracle_chain(orc, Y, U.ravel(), V.ravel(), (sw, sw // 2, sw // 2), sw, sh, 3, 0, 0, 2, 0, host(L2[0]), amounts[0], lut, None)
    assert (host(fused[0]) == want).all()


def test_chain_yuv_refusals(gpu):
    """off the one-launch form: LGPU_E_UNSUPPORTED; bad arguments: LGPU_E_BADARG; nothing is written in either case"""
    import torch
    ops = gpu
    sw, sh, dw, dh = 256, 144, 128, 72
    Y = torch.zeros((sh, sw), dtype=torch.uint8, device="cuda")
    U = torch.zeros((sh // 2, sw // 2), dtype=torch.uint8, device="cuda")
    V = torch.zeros_like(U)
    L2 = torch.zeros((dh + 8, dw * 4 + 64), dtype=torch.uint8, device="cuda")
    D = torch.full((dh + 8, dw * 4 + 64), 0x5C, dtype=torch.uint8, device="cuda")

    def call(sw_=sw, sh_=sh, dw_=dw, dh_=dh, interp=3 | PIXBUF, blur=0, amounts=(9,), canvas=None, ntracks=1, tracks=True, strides=(sw, sw // 2, sw // 2),
             usz=None, vsz=None, order=0, wt=0, q=2, flags=0, orow=dw * 4 + 64):
        prm = ops.chain_params(sw_, sh_, sw_, dw_, dh_, dw * 4 + 64, orow, swap_rb=0, interp=interp, do_blur=blur, bf=0)
        src = ops.yuv_source(strides, U.numel() if usz is None else usz, V.numel() if vsz is None else vsz, out_order=order, which_tables=wt, pb_quality=q, flags=flags)
        trk = ops.chain_yuv_tracks([Y] * max(ntracks, 1), [U] * max(ntracks, 1), [V] * max(ntracks, 1), [L2] * max(ntracks, 1), [D] * max(ntracks, 1))
        if not tracks:
            trk = (lib.ChainYuvTrack * 1)()
        am = list(amounts) * ntracks if amounts is not None else None
        trk_n = trk if ntracks >= 1 else (lib.ChainYuvTrack * 0)()
        return ops.chain_yuv420p(prm, src, trk_n, am, canvas=canvas, check=False)

    from lives_amd import lib
    unsupported = {
        "not 2:1": dict(sw_=sw + 4, strides=(sw + 4, sw // 2 + 2, sw // 2 + 2), usz=(sw // 2 + 2) * (sh // 2), vsz=(sw // 2 + 2) * (sh // 2)),
        "sw % 4 == 2": dict(sw_=2 * 127, dw_=127, strides=(254, 127, 127)),
        "odd sh": dict(sh_=143),
        "gaussian": dict(blur=1),
        "nearest": dict(interp=0 | PIXBUF),
        "odd canvas offs_x": dict(canvas=(dw + 8, dh + 4, 3, 2)),
        "destination rows not 8-byte aligned": dict(orow=dw * 4 + 4),
    }
    badarg = {
        "no PIXBUF": dict(interp=3),
        "null amounts with a blend": dict(amounts=None),
        "no tracks": dict(ntracks=0),
        "65 tracks": dict(ntracks=65),
        "null planes": dict(tracks=False),
        "out_order 2": dict(order=2),
        "which_tables 4": dict(wt=4),
        "pb_quality 0": dict(q=0),
        "unknown flag": dict(flags=2),
        "luma stride below the width": dict(strides=(sw - 4, sw // 2, sw // 2)),
        "chroma plane too small": dict(usz=U.numel() - 1),
        "canvas smaller than the frame": dict(canvas=(dw - 2, dh, 0, 0)),
        "frame outside the canvas": dict(canvas=(dw + 8, dh + 4, 10, 0)),
    }
    for what, kw in list(unsupported.items()) + list(badarg.items()):
        want = E_UNSUPPORTED if what in unsupported else E_BADARG
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc == want, "%s: %d, expected %d (%s)" % (what, rc, want, lib.last_error() if hasattr(lib, "last_error") else "")
        assert bool((D == 0x5C).all()), "%s: the destination was written" % what
    assert call() == 0      # and the same call inside the form runs
    torch.cuda.synchronize()
    assert not bool((D[:dh, :dw * 4] == 0x5C).all())
