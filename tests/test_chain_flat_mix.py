"""lgpu_chain_flat_yuv420p_mix: the unscaled tick with a decoded planar 4:2:0 frame on BOTH layers as one launch (K2's conversion of each layer under its own
lgpu_yuv_source -> [R <-> B] -> chroma blend -> [gamma LUT] -> RGBA, or -> K4's conversion to UYVY / YUYV / YUV420P; no RGBA frame anywhere) against the oracle's
composition: orc_yuv420p_to_rgb on the layer-2 planes (the chain's byte order, src2's settings) into a tight RGBA array, then tests/test_chain_flat.py's oracle_flat
with that array as layer 2.  At size also against the device's own lgpu_yuv420p_to_rgb_batch + lgpu_chain_flat_yuv420p[_to_yuv]; and the refusals.  Bit-exact: every
byte of every destination plane, and every byte of the planes' row padding and guard rows.

The CPU tests show that the GPU cases cannot pass for the wrong reason: the expectation of every case of test_mix_layer2_has_its_own_description changes when layer 2
is read through layer 1's description, and the blend amounts drawn make layer 2 visible."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.chain_ref import distinct_amounts
from tests.offset_buffers import dev_at
from tests.test_chain_flat import SMALL, UNIT_CAP, gamma_lut, oracle_flat, plane_dims, planes_any
from tests.util import align, dev, host

P = po.P
PIXBUF, NOBLEND = 0x100, 0x400
E_BADARG, E_UNSUPPORTED = -2, -3
RGBA, UYVY, YUYV, YUV420P = 0, 2, 3, 4
FIX_EDGES = 1
GUARD = 2
FMTS = [RGBA, UYVY, YUYV, YUV420P]
FMT_IDS = ["rgba", "uyvy", "yuyv", "yuv420p"]


def layer(wt=0, q=2, fix=0, pad=(0, 0, 0), tight=False, yvu=False):
    """how one layer's planes are laid out and converted: table set, pb_quality, LGPU_YUV_FIX_EDGES, row padding of the three planes, tight chroma planes (K2's read
    one past the end is clamped), and whether the planes are handed over as Y, V, U"""
    return dict(wt=wt, q=q, fix=fix, pad=pad, tight=tight, yvu=yvu)


def as_yuv(src, yvu):
    """planes_any()'s (Y, plane 1, plane 2, strides) in the order the conversion reads them"""
    Y, A1, A2, (ys_, s1, s2) = src
    return (Y, A2, A1, (ys_, s2, s1)) if yvu else (Y, A1, A2, (ys_, s1, s2))


def l2_rgba(orc, src2, sw, sh, chain_order, L, strides=None, sizes=None):
    """step 1 of the expectation: orc_yuv420p_to_rgb on the layer-2 planes into a tight RGBA array.  strides / sizes: read the same bytes through ANOTHER description
    (the CPU tests); the planes are then continued with bytes that differ from their last one, so that no read leaves the arrays"""
    Y, U, V, st = as_yuv(src2, L["yvu"])
    usz, vsz = U.size, V.size
    if strides is not None or sizes is not None:
        st = strides or st
        usz, vsz = sizes or (usz, vsz)
        room = (sh + 2) * max(max(st), src2[3][0]) + 64

        def longer(a):
            flat = a.reshape(-1)
            return np.concatenate([flat, np.full(room, flat[-1] ^ 0xFF, np.uint8)])
        Y, U, V = longer(Y), longer(U), longer(V)
    rgba = np.zeros((sh, sw * 4), np.uint8)
    orc.orc_yuv420p_to_rgb(P(Y), P(U), P(V), (ctypes.c_int * 3)(*st), usz, vsz, P(rgba), sw * 4, sw, sh, 4, chain_order, 0, L["wt"], L["q"], None, L["fix"])
    return rgba


def expected_mix(orc, src1, src2, sw, sh, order, swap, L1, L2, amount, lut, fmt, wt_sink, l2=None):
    """the destination planes one track must equal; l2: a layer-2 RGBA array made some other way (the CPU tests)"""
    if l2 is None:
        l2 = l2_rgba(orc, src2, sw, sh, order ^ swap, L2)
    Y, U, V, st = as_yuv(src1, L1["yvu"])
    return oracle_flat(orc, Y, U, V, st, sw, sh, order, swap, L1["wt"], L1["q"], L1["fix"], l2, amount, lut, None, fmt, wt_sink)


def source_of(ops, src, L, order):
    _, U, V, st = as_yuv(src, L["yvu"])
    return ops.yuv_source(st, U.size, V.size, out_order=order, which_tables=L["wt"], pb_quality=L["q"], flags=L["fix"])


def run_mix(gpu, orc, rng, sw, sh, fmt=RGBA, ntracks=1, lut=None, order=0, swap=0, L1=None, L2=None, wt_sink=0, yvu_sink=False, pads=(8, 3, 5), dst_off=0, l2_offs=None,
            srcs=None, srcs2=None, amounts=None, itself=False):
    """one call with ntracks tracks that all differ; the device buffers are allocated in a shuffled order and handed over in another (slot order != frame order);
    every destination plane is compared whole: frame bytes against the oracle, row padding and guard rows against their fill.  dst_off: the address of the first
    destination plane modulo 64; l2_offs: the addresses of layer 2's three planes modulo 64 (None: wherever the allocator puts them); itself: layer 2's pointers are
    layer 1's"""
    ops = gpu
    L1, L2 = L1 or layer(), L2 or layer()
    dims = plane_dims(fmt, sw, sh)
    strides = [align(b + pads[k], 4 if fmt in (RGBA, UYVY, YUYV) else 2 if k == 0 else 1) for k, (b, _) in enumerate(dims)]
    srcs = srcs if srcs is not None else [planes_any(rng, sw, sh, L1["pad"], L1["tight"]) for _ in range(ntracks)]
    if itself:
        srcs2 = srcs
    srcs2 = srcs2 if srcs2 is not None else [planes_any(rng, sw, sh, L2["pad"], L2["tight"]) for _ in range(ntracks)]
    amounts = amounts if amounts is not None else distinct_amounts(rng, ntracks)
    fills = [[rng.integers(0, 256, (r + GUARD, strides[k]), dtype=np.uint8) for k, (_, r) in enumerate(dims)] for _ in range(ntracks)]
    d_src, d_src2, d_pl = [None] * ntracks, [None] * ntracks, [None] * ntracks
    for i in rng.permutation(ntracks):
        d_pl[i] = [dev_at(f, dst_off if k == 0 else 0) for k, f in enumerate(fills[i])]
        if l2_offs is not None and not itself:
            d_src2[i] = [dev_at(np.ascontiguousarray(p).reshape(1, -1) if p.ndim == 1 else p, l2_offs[j]) for j, p in enumerate(srcs2[i][:3])]
        d_src[i] = [dev(p) for p in srcs[i][:3]]
        if itself:
            d_src2[i] = d_src[i]
        elif l2_offs is None:
            d_src2[i] = [dev(p) for p in srcs2[i][:3]]
    slots = [int(k) for k in rng.permutation(ntracks)]
    s1 = [0, 2, 1] if L1["yvu"] else [0, 1, 2]
    s2 = [0, 2, 1] if L2["yvu"] else [0, 1, 2]
    dsel = [0, 2, 1] if (yvu_sink and fmt == YUV420P) else list(range(len(dims)))
    prm = ops.chain_params(sw, sh, 0, sw, sh, 0, strides[0] if fmt == RGBA else 0, swap_rb=swap, interp=PIXBUF, bf=0, lut=lut)
    src, src2 = source_of(ops, srcs[0], L1, order), source_of(ops, srcs2[0], L2, order ^ swap)
    sink = ops.chain_sink(fmt, [strides[j] for j in dsel], which_tables=wt_sink, in_order=order ^ swap) if fmt != RGBA else None
    trk = ops.chain_yuv_mix_tracks([d_src[k][s1[0]] for k in slots], [d_src[k][s1[1]] for k in slots], [d_src[k][s1[2]] for k in slots],
                                   [d_src2[k][s2[0]] for k in slots], [d_src2[k][s2[1]] for k in slots], [d_src2[k][s2[2]] for k in slots],
                                   [[d_pl[k][j] for j in dsel] for k in slots])
    ops.chain_flat_yuv420p_mix(prm, src, src2, trk, [amounts[k] for k in slots], sink=sink)
    wants = []
    for i in range(ntracks):
        want = expected_mix(orc, srcs[i], srcs2[i], sw, sh, order, swap, L1, L2, amounts[i], lut, fmt, wt_sink)
        wants.append(want)
        for p, j in enumerate(dsel):              # p: the conversion's plane (Y, U, V); j: the buffer it was handed
            b, r = dims[p]
            got = host(d_pl[i][j])
            bad = got[:r, :b] != want[p][:r, :b]
            assert not bad.any(), "%dx%d fmt %d track %d plane %d: %d bytes differ from the oracle, first at %s" % (sw, sh, fmt, i, p, int(bad.sum()), np.argwhere(bad)[0].tolist())
            assert (got[:r, b:] == fills[i][j][:r, b:]).all(), "track %d plane %d: row padding was written" % (i, p)
            assert (got[r:] == fills[i][j][r:]).all(), "track %d plane %d: guard rows were written" % (i, p)
    return wants


def drawn_layer(rng, i):
    return layer(wt=int(rng.integers(0, 4)), q=int(rng.integers(1, 4)), fix=int(rng.integers(0, 2)) * FIX_EDGES, pad=(int(rng.integers(0, 6)), int(rng.integers(0, 6)), 1 + 2 * i),
                 tight=bool(rng.integers(0, 2)), yvu=bool(rng.integers(0, 2)))


@pytest.mark.gpu
@pytest.mark.parametrize("with_lut", [True, False], ids=["lut", "nolut"])
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_mix_stages(gpu, orc, fmt, with_lut):
    """every destination with and without the LUT, both settings of swap_rb, two tracks; layer 1's out_order (layer 2's is then src->out_order ^ swap_rb, the only one
    the entry point takes), and per layer and independently: table set, pb_quality, LGPU_YUV_FIX_EDGES, pitches, tight planes, the U / V plane order; the sink's plane
    order and tables drawn too"""
    rng = np.random.default_rng(0x313 + fmt * 2 + with_lut)
    lut = gamma_lut(orc) if with_lut else None
    for i, (sw, sh) in enumerate([(132, 76), (36, 21) if fmt != YUV420P else (36, 22)]):
        for swap in (0, 1):
            wt_sink = int(rng.integers(0, 4)) if fmt == YUV420P else int(rng.integers(0, 2))
            run_mix(gpu, orc, rng, sw, sh, fmt, ntracks=2, lut=lut, order=int(rng.integers(0, 2)), swap=swap, L1=drawn_layer(rng, i), L2=drawn_layer(rng, i), wt_sink=wt_sink,
                    yvu_sink=bool(rng.integers(0, 2)), pads=(8 * i, 3 + 2 * i, 7))


@pytest.mark.gpu
@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("sw,sh", SMALL)
def test_mix_smallest_frames_rgba(gpu, orc, sw, sh, fix):
    """the walk's smallest frames on both layers into RGBA and the packed sinks: row 0 alone, with and without a row pair, with and without the trailing row, chroma
    widths 65 and 66; layer 2 with fix_edges = fix and layer 1 with the other setting; tight and loose chroma planes"""
    rng = np.random.default_rng(0x5A12 + sw * 131 + sh * 2 + fix)
    lut = gamma_lut(orc)
    for tight in (True, False):
        run_mix(gpu, orc, rng, sw, sh, RGBA, ntracks=2, lut=lut, swap=fix, L1=layer(fix=1 - fix, q=3 - fix, pad=(1, 1, 3), tight=tight), L2=layer(fix=fix, q=2 + fix, pad=(3, 1, 1), tight=not tight))
        run_mix(gpu, orc, rng, sw, sh, UYVY if tight else YUYV, ntracks=2, lut=lut, order=1, L1=layer(fix=1 - fix, q=2, pad=(3, 1, 1), tight=tight), L2=layer(fix=fix, q=1 + fix, pad=(1, 3, 1), tight=tight))


@pytest.mark.gpu
@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("sw,sh", [g for g in SMALL if not g[1] & 1] + [(2, 4)])
def test_mix_smallest_frames_yuv420p(gpu, orc, sw, sh, fix):
    """the 4:2:0 sink on the even heights of the list and 2x4 (one inner row pair between row 0 and the trailing row); layer 2 with fix_edges = fix, layer 1 with the
    other setting"""
    rng = np.random.default_rng(0x421 + sw * 131 + sh * 2 + fix)
    for tight in (True, False):
        run_mix(gpu, orc, rng, sw, sh, YUV420P, ntracks=2, lut=gamma_lut(orc), L1=layer(fix=1 - fix, pad=(1, 3, 1), tight=tight), L2=layer(fix=fix, wt=1, pad=(1, 1, 3), tight=not tight),
                wt_sink=int(tight) * 2 + fix, pads=(2, 1, 3))


# ---- layer 2 is read through its own description: each case differs between the layers in exactly one respect; (what, layer 1, layer 2, sh); run both ways round
OWN_CASES = [
    ("pitches", layer(pad=(1, 1, 3)), layer(pad=(4, 5, 0)), 21),
    ("sizes", layer(pad=(1, 1, 3), tight=True), layer(pad=(1, 1, 3), tight=False), 21),
    ("tables 0/1", layer(wt=0), layer(wt=1), 21),
    ("tables 0/2", layer(wt=0), layer(wt=2), 21),
    ("tables 0/3", layer(wt=0), layer(wt=3), 21),
    ("quality", layer(q=1), layer(q=2), 21),
    ("fix_edges", layer(fix=FIX_EDGES), layer(fix=0), 22),      # an even height: the flag only acts on the trailing row
]
OWN_IDS = [c[0].replace(" ", "_").replace("/", "_") for c in OWN_CASES]
OWN_W = 36


def own_case(case, way):
    """the inputs of one case and direction, the same on the GPU and on the CPU: two tracks with amounts 0 and 255"""
    what, La, Lb, sh = OWN_CASES[case]
    L1, L2 = (La, Lb) if way == 0 else (Lb, La)
    rng = np.random.default_rng(0x0A17 + case * 2 + way)
    srcs = [planes_any(rng, OWN_W, sh, L1["pad"], L1["tight"]) for _ in range(2)]
    srcs2 = [planes_any(rng, OWN_W, sh, L2["pad"], L2["tight"]) for _ in range(2)]
    return what, L1, L2, sh, srcs, srcs2, distinct_amounts(rng, 2), rng


@pytest.mark.gpu
@pytest.mark.parametrize("way", [0, 1])
@pytest.mark.parametrize("case", range(len(OWN_CASES)), ids=OWN_IDS)
def test_mix_layer2_has_its_own_description(gpu, orc, case, way):
    """pitches, chroma plane sizes (the clamp of the read past the end), table set, LOW quality and FIX_EDGES on one layer only, both ways round, to RGBA and to a packed
    sink (test_mix_expectation_needs_layer2s_own_description shows on the CPU that reading layer 2 through layer 1's description would change these expectations)"""
    what, L1, L2, sh, srcs, srcs2, amounts, rng = own_case(case, way)
    run_mix(gpu, orc, rng, OWN_W, sh, RGBA, ntracks=2, L1=L1, L2=L2, srcs=srcs, srcs2=srcs2, amounts=amounts)
    run_mix(gpu, orc, rng, OWN_W, sh, YUYV, ntracks=2, lut=gamma_lut(orc), order=1, L1=L1, L2=L2, srcs=srcs, srcs2=srcs2, amounts=amounts)


@pytest.mark.parametrize("way", [0, 1])
@pytest.mark.parametrize("case", range(len(OWN_CASES)), ids=OWN_IDS)
def test_mix_expectation_needs_layer2s_own_description(orc, case, way):
    """for the seeds and amounts of the GPU test above: the oracle's expectation changes when layer 2 is described with layer 1's pitches, sizes, tables, quality or
    flag instead of its own"""
    what, L1, L2, sh, srcs, srcs2, amounts, _ = own_case(case, way)
    i = amounts.index(255)
    right = expected_mix(orc, srcs[i], srcs2[i], OWN_W, sh, 0, 0, L1, L2, 255, None, RGBA, 0)[0]
    _, U1, V1, st1 = as_yuv(srcs[i], L1["yvu"])
    if what == "pitches":
        wrong_l2 = l2_rgba(orc, srcs2[i], OWN_W, sh, 0, L2, strides=st1)
    elif what == "sizes":
        wrong_l2 = l2_rgba(orc, srcs2[i], OWN_W, sh, 0, L2, sizes=(U1.size, V1.size))
    else:
        key = {"tables": "wt", "quality": "q", "fix_edges": "fix"}[what.split(" ")[0]]
        assert L1[key] != L2[key]
        wrong_l2 = l2_rgba(orc, srcs2[i], OWN_W, sh, 0, dict(L2, **{key: L1[key]}))
    wrong = expected_mix(orc, srcs[i], srcs2[i], OWN_W, sh, 0, 0, L1, L2, 255, None, RGBA, 0, l2=wrong_l2)[0]
    assert (right != wrong).any(), "%s: layer 2 read through layer 1's description gives the same bytes; the GPU case would not tell them apart" % what


def test_mix_amounts_make_layer2_visible(orc):
    """distinct_amounts() draws 0 and 255 once there are two tracks.  With amount 0 layer 2 does not reach the result: the expectation is the same for any layer 2,
    and it is the blend's own (255 * c) >> 8 of the frame without a layer 2 (simple_blend's integer expression has no identity at 0).  With 255 layer 2 does reach
    it, and so it does at the other amounts the tests draw"""
    rng = np.random.default_rng(0xA0)
    sw, sh = 36, 21
    L = layer(pad=(1, 1, 3))
    src, src2, other = (planes_any(rng, sw, sh, L["pad"], False) for _ in range(3))
    assert distinct_amounts(rng, 2) == [0, 255] and set(distinct_amounts(rng, 9)[:2]) == {0, 255}
    for fmt in (RGBA, UYVY):
        none = expected_mix(orc, src, src2, sw, sh, 0, 0, L, L, 0, None, fmt, 0)[0]
        assert (none == expected_mix(orc, src, other, sw, sh, 0, 0, L, L, 0, None, fmt, 0)[0]).all()
        for amount in (255, 1, 128):
            assert (expected_mix(orc, src, src2, sw, sh, 0, 0, L, L, amount, None, fmt, 0)[0] != expected_mix(orc, src, other, sw, sh, 0, 0, L, L, amount, None, fmt, 0)[0]).any()
    Y, U, V, st = as_yuv(src, False)
    alone = oracle_flat(orc, Y, U, V, st, sw, sh, 0, 0, 0, 2, 0, None, 0, None)[0].reshape(sh, sw, 4).astype(np.int32)
    want = (alone * 255) >> 8
    want[:, :, 3] = alone[:, :, 3]
    assert (expected_mix(orc, src, src2, sw, sh, 0, 0, L, L, 0, None, RGBA, 0)[0].reshape(sh, sw, 4) == want).all()


def test_mix_track_struct_size():
    from lives_amd import lib
    assert ctypes.sizeof(lib.ChainYuvMixTrack) == 72


@pytest.mark.gpu
@pytest.mark.parametrize("ntracks", [1, 7, 16, 32, 33, 64])
def test_mix_tracks(gpu, orc, ntracks):
    """1 .. 64 tracks in one call with distinct amounts (0 and 255 among them) and shuffled buffers, to every destination; 32 tracks per launch, so 33 and 64 go as
    two"""
    rng = np.random.default_rng(0x7AD + ntracks)
    lut = gamma_lut(orc)
    sw, sh = 68, 10
    run_mix(gpu, orc, rng, sw, sh, RGBA, ntracks=ntracks, lut=lut, swap=1, L1=layer(wt=1, pad=(4, 1, 3)), L2=layer(wt=1, pad=(0, 3, 1)))
    run_mix(gpu, orc, rng, sw, sh, YUV420P, ntracks=ntracks, lut=lut, order=1, L1=layer(wt=2, pad=(4, 0, 2)), L2=layer(wt=3, pad=(2, 2, 0), yvu=True), wt_sink=2, yvu_sink=True)
    run_mix(gpu, orc, rng, sw, sh, UYVY, ntracks=ntracks, lut=lut, swap=1, L1=layer(), L2=layer(q=1, tight=True))
    run_mix(gpu, orc, rng, sw, sh, YUYV, ntracks=ntracks, order=1, L1=layer(yvu=True), L2=layer(fix=FIX_EDGES), wt_sink=1)


@pytest.mark.gpu
@pytest.mark.parametrize("dst_off", [4, 12])
def test_mix_addresses(gpu, orc, dst_off):
    """destination at 4 and 12 mod 16 with pitches of 4 mod 8 (RGBA, UYVY): 4-byte stores where the address is not a multiple of 8; 4:2:0 luma at 2 mod 4 with odd
    chroma pitches; layer 2's luma and chroma planes at odd addresses with odd pitches"""
    rng = np.random.default_rng(0xADE + dst_off)
    L2 = layer(pad=(1, 3, 1), wt=1)
    assert (132 * 4 + 4) % 8 == 4 and (132 * 2 + 4) % 8 == 4 and (132 + 1) % 2 == 1 and (66 + 3) % 2 == 1 and (66 + 1) % 2 == 1
    run_mix(gpu, orc, rng, 132, 8, RGBA, ntracks=2, lut=gamma_lut(orc), L2=L2, dst_off=dst_off, l2_offs=(1, 3, 5), pads=(4, 0, 0))
    run_mix(gpu, orc, rng, 132, 8, UYVY, ntracks=2, L2=L2, dst_off=dst_off, l2_offs=(3, 1, 7), pads=(4, 0, 0))
    run_mix(gpu, orc, rng, 132, 8, YUV420P, ntracks=2, L2=L2, dst_off=dst_off + 2, l2_offs=(5, 7, 1), pads=(2, 1, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_mix_wide_and_tall(gpu, orc, fmt):
    """1100 pixels: 550 chroma columns, three workgroups along x with the last one partly empty; a frame of width 4 with more units than a launch's workgroup rows
    (each workgroup then walks a run of units) and one with a few units more than workgroups; layer 2 with fix_edges opposite to layer 1"""
    rng = np.random.default_rng(0x71DF + fmt)
    run_mix(gpu, orc, rng, 1100, 10 if fmt == YUV420P else 9, fmt, lut=gamma_lut(orc), L1=layer(tight=True, pad=(0, 1, 1)), L2=layer(fix=FIX_EDGES, pad=(2, 0, 3)))
    run_mix(gpu, orc, rng, 4, 2 * UNIT_CAP + 6, fmt, L1=layer(fix=FIX_EDGES, pad=(1, 1, 1)), L2=layer(wt=1, pad=(0, 1, 0), tight=True))
    run_mix(gpu, orc, rng, 4, 4 * UNIT_CAP + 2, fmt, ntracks=2, lut=gamma_lut(orc), L1=layer(tight=True), L2=layer(fix=FIX_EDGES, pad=(3, 0, 1)))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [RGBA, UYVY, YUV420P], ids=["rgba", "uyvy", "yuv420p"])
def test_mix_at_size_matches_todays_launches(gpu, orc, fmt):
    """4 x 1920x1080 with blend and gamma: byte-identical to the device's own lgpu_yuv420p_to_rgb_batch on layer 2 followed by lgpu_chain_flat_yuv420p[_to_yuv] on the
    same inputs; track 0 also against the oracle"""
    import torch
    ops = gpu
    rng = np.random.default_rng(0x52 + fmt)
    w, h, n = 1920, 1080, 4
    lut = gamma_lut(orc)
    g = torch.Generator(device="cuda")
    g.manual_seed(8643 + fmt)

    def rnd(shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
    Ys, Us, Vs = [rnd((h, w)) for _ in range(n)], [rnd((h // 2, w // 2)) for _ in range(n)], [rnd((h // 2, w // 2)) for _ in range(n)]
    Y2, U2, V2 = [rnd((h, w)) for _ in range(n)], [rnd((h // 2, w // 2)) for _ in range(n)], [rnd((h // 2, w // 2)) for _ in range(n)]
    amounts = [int(x) for x in rng.integers(1, 256, n)]
    dims = plane_dims(fmt, w, h)
    fused = [[torch.full((r, b), 0x5C, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
    today = [[torch.full((r, b), 0xC5, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
    prm = ops.chain_params(w, h, w * 4, w, h, w * 4, w * 4, swap_rb=1, interp=PIXBUF, bf=0, lut=lut)
    src = ops.yuv_source((w, w // 2, w // 2), Us[0].numel(), Vs[0].numel(), out_order=0, which_tables=0, pb_quality=2)
    src2 = ops.yuv_source((w, w // 2, w // 2), U2[0].numel(), V2[0].numel(), out_order=1, which_tables=1, pb_quality=3, flags=FIX_EDGES)
    sink = ops.chain_sink(fmt, [b for (b, _) in dims], which_tables=0, in_order=1) if fmt != RGBA else None
    ops.chain_flat_yuv420p_mix(prm, src, src2, ops.chain_yuv_mix_tracks(Ys, Us, Vs, Y2, U2, V2, fused), amounts, sink=sink)
    conv = [torch.zeros((h, w * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    ops.yuv420p_to_rgb_batch(list(zip(Y2, U2, V2, conv)), w, h, 4, 1, 0, 1, 3, flags=FIX_EDGES)
    if fmt == RGBA:
        ops.chain_flat_yuv420p(prm, src, ops.chain_yuv_tracks(Ys, Us, Vs, conv, [t[0] for t in today]), amounts)
    else:
        ops.chain_flat_yuv420p_to_yuv(prm, src, sink, ops.chain_yuv_sink_tracks(Ys, Us, Vs, conv, today), amounts)
    torch.cuda.synchronize()
    for i in range(n):
        for p in range(len(dims)):
            assert torch.equal(fused[i][p], today[i][p]), "track %d plane %d: %d bytes differ from today's launches" % (i, p, int((fused[i][p] != today[i][p]).sum()))
    hw = w // 2
    s1 = (host(Ys[0]), host(Us[0]).reshape(-1), host(Vs[0]).reshape(-1), (w, hw, hw))
    s2 = (host(Y2[0]), host(U2[0]).reshape(-1), host(V2[0]).reshape(-1), (w, hw, hw))
    want = expected_mix(orc, s1, s2, w, h, 0, 1, layer(), layer(wt=1, q=3, fix=FIX_EDGES), amounts[0], lut, fmt, 0)
    for p, (b, r) in enumerate(dims):
        assert (host(fused[0][p]) == want[p][:r, :b]).all(), "track 0 plane %d differs from the oracle" % p


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_mix_a_clip_with_itself(gpu, orc, fmt):
    """layer 2's pointers are layer 1's, amount 128: the same planes under the same description, and under another table set and quality"""
    rng = np.random.default_rng(0x5E1F + fmt)
    sh = 22 if fmt == YUV420P else 21
    run_mix(gpu, orc, rng, 36, sh, fmt, ntracks=2, lut=gamma_lut(orc), L1=layer(pad=(1, 1, 3)), L2=layer(pad=(1, 1, 3)), amounts=[128, 128], itself=True)
    run_mix(gpu, orc, rng, 36, sh, fmt, swap=1, L1=layer(pad=(1, 1, 3)), L2=layer(pad=(1, 1, 3), wt=1, q=1), amounts=[128], itself=True)


@pytest.mark.gpu
def test_mix_refusals(gpu):
    """every LGPU_E_BADARG and LGPU_E_UNSUPPORTED item of the entry point, one call each: the code is compared and the destinations' fill is still whole afterwards;
    the same call inside the form then runs (its bytes are test_mix_stages' business; here: it wrote the frame and nothing else)"""
    import torch
    from lives_amd import lib
    ops = gpu
    w, h = 128, 72
    Y = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    U = torch.zeros((h // 2, w // 2), dtype=torch.uint8, device="cuda")
    V = torch.zeros_like(U)
    Y2, U2, V2 = torch.full_like(Y, 200), torch.full_like(U, 90), torch.full_like(V, 160)
    D = [torch.full((h + 16, w * 4 + 64), 0x5C, dtype=torch.uint8, device="cuda") for _ in range(3)]
    full = (w, w // 2, w // 2)

    def call(fmt=YUV420P, sw_=w, sh_=h, dw_=None, dh_=None, interp=PIXBUF, blur=0, amounts=(9,), ntracks=1, null=None, null_plane=False, strides=full, strides2=full,
             usz=None, vsz=None, usz2=None, vsz2=None, order=0, order2=None, swap=0, wt_src=0, wt_src2=0, q=2, q2=2, flags=0, flags2=0, wt=0, in_order=None, orow=None, dst_off=0,
             in_place=None, no_src2=False):
        dw_, dh_ = sw_ if dw_ is None else dw_, sh_ if dh_ is None else dh_
        orow = orow if orow is not None else [w * 4 + 64] * 3
        prm = ops.chain_params(sw_, sh_, 0, dw_, dh_, 0, orow[0], swap_rb=swap, interp=interp, do_blur=blur, bf=0)
        src = ops.yuv_source(strides, U.numel() if usz is None else usz, V.numel() if vsz is None else vsz, out_order=order, which_tables=wt_src, pb_quality=q, flags=flags)
        src2 = ops.yuv_source(strides2, U2.numel() if usz2 is None else usz2, V2.numel() if vsz2 is None else vsz2, out_order=(order ^ swap) if order2 is None else order2,
                              which_tables=wt_src2, pb_quality=q2, flags=flags2)
        m = max(ntracks, 1)
        sink = ops.chain_sink(fmt, orow, which_tables=wt, in_order=(order ^ swap) if in_order is None else in_order) if fmt != RGBA else None
        trk = ops.chain_yuv_mix_tracks([Y] * m, [U] * m, [V] * m, [Y2] * m, [U2] * m, [V2] * m, [D] * m)
        for t in trk:
            t.dst_d[0] += dst_off
        if null is not None:
            setattr(trk[0], null, None)
        if null_plane:
            trk[0].dst_d[2 if fmt == YUV420P else 0] = None
        if in_place is not None:
            trk[0].dst_d[in_place[0]] = (Y, U, V, Y2, U2, V2)[in_place[1]].data_ptr()
        if ntracks < 1:
            trk = (lib.ChainYuvMixTrack * 0)()
        args = (ctypes.byref(prm), ctypes.byref(src), None if no_src2 else ctypes.byref(src2), ctypes.byref(sink) if sink is not None else None, trk, len(trk),
                (ctypes.c_uint8 * m)(*(list(amounts) * m)) if amounts is not None else None, ops.stream_ptr())
        if no_src2:
            return lib.load().lgpu_chain_flat_yuv420p_mix(*args)
        return ops.chain_flat_yuv420p_mix(prm, src, src2, trk, list(amounts) * m if amounts is not None else None, sink=sink, check=False)

    both_badarg = {
        "no PIXBUF": dict(interp=3),
        "NOBLEND": dict(interp=PIXBUF | NOBLEND),
        "NOBLEND and null amounts": dict(interp=PIXBUF | NOBLEND, amounts=None),
        "null amounts": dict(amounts=None),
        "no tracks": dict(ntracks=0),
        "65 tracks": dict(ntracks=65),
        "null src2": dict(no_src2=True),
        "null layer-1 plane": dict(null="u_d"),
        "null layer-2 luma plane": dict(null="y2_d"),
        "null layer-2 U plane": dict(null="u2_d"),
        "null layer-2 V plane": dict(null="v2_d"),
        "null destination plane": dict(null_plane=True),
        "out_order 2": dict(order=2, order2=0, in_order=0),
        "src2 out_order 2": dict(order2=2),
        "src2 out_order against the chain's (no swap)": dict(order=1, swap=0, order2=0),
        "src2 out_order against the chain's (swap)": dict(order=1, swap=1, order2=1),
        "source which_tables 4": dict(wt_src=4),
        "src2 which_tables 4": dict(wt_src2=4),
        "src2 which_tables -1": dict(wt_src2=-1),
        "pb_quality 0": dict(q=0),
        "src2 pb_quality 0": dict(q2=0),
        "src2 pb_quality 4": dict(q2=4),
        "unknown flag": dict(flags=2),
        "src2 unknown flag": dict(flags2=2),
        "luma stride below the width": dict(strides=(w - 4, w // 2, w // 2)),
        "src2 luma stride below the width": dict(strides2=(w - 4, w // 2, w // 2)),
        "chroma stride below the width": dict(strides=(w, w // 2 - 2, w // 2)),
        "src2 U stride below the width": dict(strides2=(w, w // 2 - 2, w // 2)),
        "src2 V stride below the width": dict(strides2=(w, w // 2, w // 2 - 2)),
        "chroma plane too small": dict(usz=U.numel() - 1),
        "src2 U plane too small": dict(usz2=U.numel() - 1),
        "src2 V plane too small": dict(vsz2=V.numel() - 1),
        "odd sw": dict(sw_=127),
        "sw 0": dict(sw_=0),
        "sh 0": dict(sh_=0),
        "dw 0": dict(dw_=0),
        "destination is layer 1's luma plane": dict(in_place=(0, 0)),
        "destination is layer 1's V plane": dict(in_place=(0, 2)),
        "destination is layer 2's luma plane": dict(in_place=(0, 3)),
        "destination is layer 2's U plane": dict(in_place=(0, 4)),
        "destination is layer 2's V plane": dict(in_place=(0, 5)),
    }
    rgba_badarg = {
        "destination stride below the row": dict(orow=[w * 4 - 4] * 3),
        "destination stride not a multiple of 4": dict(orow=[w * 4 + 2] * 3),
        "destination not 4-byte aligned": dict(dst_off=2),
    }
    sink_badarg = {
        "out_fmt 1": dict(fmt=1),
        "out_fmt 6": dict(fmt=6),
        "in_order 2": dict(in_order=2),
        "sink which_tables 4": dict(wt=4),
        "BT.709 with UYVY": dict(fmt=UYVY, wt=2),
        "BT.709 with YUYV": dict(fmt=YUYV, wt=3),
        "sink luma stride below the row": dict(orow=[w - 8, w, w]),
        "sink chroma stride below the row": dict(orow=[w, w // 2 - 4, w]),
        "packed stride below the row": dict(fmt=UYVY, orow=[w * 2 - 8, 0, 0]),
        "in_order against the chain's (no swap)": dict(order=1, swap=0, in_order=0),
        "in_order against the chain's (swap)": dict(order=1, swap=1, in_order=1),
        "chroma sink plane is layer 1's V plane": dict(in_place=(1, 2)),
        "chroma sink plane is layer 2's U plane": dict(in_place=(2, 4)),
    }
    both_unsupported = {
        "2:1": dict(dw_=w // 2, dh_=h // 2),
        "another width": dict(dw_=w + 2),
        "another height": dict(dh_=h - 1),
        "gaussian": dict(blur=1),
        "luma plane of 2 GiB": dict(strides=(1 << 25, w // 2, w // 2)),
        "chroma plane of 2 GiB": dict(usz=1 << 31),
        "layer-2 luma plane of 2 GiB": dict(strides2=(1 << 25, w // 2, w // 2)),
        "layer-2 U plane of 2 GiB": dict(usz2=1 << 31),
        "layer-2 V plane of 2 GiB": dict(vsz2=1 << 31),
    }
    sink_unsupported = {
        "YUV422P": dict(fmt=5),
        "odd dh with 4:2:0": dict(sh_=71),
        "odd luma rowstride": dict(orow=[w + 1, w, w]),
        "odd luma plane": dict(dst_off=1),
        "packed rowstride % 4 == 2": dict(fmt=YUYV, orow=[w * 2 + 2, 0, 0]),
        "packed plane at 2 mod 4": dict(fmt=UYVY, dst_off=2),
    }
    cases = []
    for fmt in (RGBA, YUV420P):
        cases += [(what, dict(fmt=fmt, **kw), E_BADARG) for what, kw in both_badarg.items()]
        cases += [(what, dict(fmt=fmt, **kw), E_UNSUPPORTED) for what, kw in both_unsupported.items()]
    cases += [(what, dict(fmt=RGBA, **kw), E_BADARG) for what, kw in rgba_badarg.items()]
    cases += [(what, kw, E_BADARG) for what, kw in sink_badarg.items()]
    cases += [(what, kw, E_UNSUPPORTED) for what, kw in sink_unsupported.items()]
    for what, kw, want in cases:
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc == want, "%s (%s): %d, expected %d (%s)" % (what, kw, rc, want, lib.load().lgpu_last_error())
        assert all(bool((d == 0x5C).all()) for d in D), "%s: a destination plane was written" % what
    # ... and the same calls inside the form run
    assert call(fmt=UYVY, sh_=71) == 0                 # any height for the packed formats
    torch.cuda.synchronize()
    assert not bool((D[0][:71, :w * 2] == 0x5C).all()) and bool((D[0][71:] == 0x5C).all()) and bool((D[0][:, w * 2:] == 0x5C).all()) and bool((D[1] == 0x5C).all())
    assert call(order=1, swap=1) == 0
    torch.cuda.synchronize()
    assert not bool((D[0][:h, :w] == 0x5C).all()) and not any(bool((d[:h // 2, :w // 2] == 0x5C).all()) for d in D[1:])
    for d in D:
        d.fill_(0x5C)
    assert call(fmt=RGBA, sh_=71, amounts=(128,)) == 0
    torch.cuda.synchronize()
    assert not bool((D[0][:71, :w * 4] == 0x5C).all()) and bool((D[0][71:] == 0x5C).all()) and bool((D[0][:, w * 4:] == 0x5C).all()) and bool((D[1] == 0x5C).all())
