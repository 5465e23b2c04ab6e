"""Launches of 17 to 64 tracks (LGPU_CHAIN_MAX_TRACKS) on every multi-track entry point, each track against the oracle (or, where a test says so, against its own
one-track call), guard rows and row padding of every destination checked: lgpu_chain_amounts and lgpu_chain_yuv420p on the exact 2:1 kernel (k_pb_half, whose
track index is decoded from a flattened, XCD-dealt workgroup id in two work orders), the chain off 2:1 on the ratio scalers, the staged walk with its scratch groups,
the polyphase chain (k_half8s' persistent walk crosses tracks within one stride; k_sep2p's tile list), lgpu_pixbuf_scale_batch, lgpu_yuv420p_to_rgb_batch, and the
refusal of 65 tracks.  Every case names the launch shape it is meant to reach, and a restatement of the planner's rules checks that it does reach it on this device."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.chain_ref import Tracks, distinct_amounts, oracle_chain, oracle_chain_rgba, planes
from tests.util import align, dev, host

pytestmark = pytest.mark.gpu
P = po.P
PIXBUF, NOBLEND = 0x100, 0x400
E_BADARG = -2


def cdiv(a, b):
    return (a + b - 1) // b


def device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def pbh_plan(dw, dh, ntracks, yuv=False, aligned=None, th=None, order=None, group=None):
    """pb_half_geometry's band count and pb_chain_half's / lgpu_chain_yuv420p's work order and band group, restated (pixbuf.hip) for the device's CU count:
    -> dict(order, bgroup, bands, cgroups).  order / group: what PBH_ORDER / PBH_GROUP force (the 4:2:0 entry point ignores both)"""
    cus = device_cus()
    aligned = 0 if yuv else (1 if aligned is None else aligned)
    strips = cdiv(dw, 128 if aligned else 124)
    cgroups = (strips + 3) // 4
    bands = cdiv(dh, 6)
    if cgroups * ntracks * bands > cus * 8:
        bands = 8 * max(1, (dh + 20) // 40)
    if th:
        bands = cdiv(dh, th)
    bands = max(1, min(bands, dh))
    if yuv or order is None:
        order = 2 if cgroups * bands * ntracks >= cus * 8 + 1 else 1
    if yuv or group is None:
        group = bands // 8 if bands % 8 == 0 else 1
    return dict(order=order, bgroup=group, bands=bands, cgroups=cgroups)


def reach(plan, claim, what):
    got = {k: plan[k] for k in claim}
    assert got == claim, "%s: the planner gives %s on this device (%d CUs), the case claims %s" % (what, got, device_cus(), claim)


def gamma_lut(rng):
    return rng.permutation(256).astype(np.uint8)


class Switches:
    """launch-shape switches for one launch: set, then every one touched back to unset"""

    def __init__(self, tune):
        self.tune, self.names = tune, set()

    def set(self, sw):
        for name in self.names - set(sw):
            self.tune(name, None)
        for name, v in sw.items():
            self.tune(name, v)
        self.names |= set(sw)


# ---------------------------------------------------------------- a. lgpu_chain_amounts, pixbuf 2:1, one launch (k_pb_half)

# (tracks, sw, sh, the planner's shape with no switch set, what PBH_TH = 5 gives)
A_GEOM = [(17, 260, 146, dict(order=1, bands=13), dict(order=1, bands=15)),
          (33, 512, 288, dict(order=1, bands=24), dict(order=1, bands=29)),
          (64, 1024, 576, dict(order=2, bgroup=7, bands=56), dict(order=2, bgroup=1, bands=58))]
A_STAGES = [(True, False, True), (False, False, False), (True, True, False), (False, True, True)]        # (blend, canvas, LUT)
A_SWITCHES = [{}] + [dict(PBH_ORDER=o, **({"PBH_GROUP": g} if g else {})) for o in (1, 2) for g in (1, 3, None)] + [dict(PBH_TH=5)]


@pytest.mark.parametrize("stages", A_STAGES, ids=["blend-lut", "noblend", "canvas-blend", "canvas-noblend-lut"])
@pytest.mark.parametrize("geom", A_GEOM, ids=["17x260x146", "33x512x288", "64x1024x576"])
def test_chain_amounts_half(gpu, orc, tune, geom, stages):
    """17 x 260x146 (13 bands) and 33 x 512x288 (24 bands) reach work order 1; 64 x 1024x576 reaches order 2 with 56 bands in groups of 7, and with PBH_TH = 5
    58 bands (not a multiple of 8: bgroup 1) -- under both strip forms (PBH_ALIGNED 0 / 1), then every order forced with bgroup 1, 3 and the planner's"""
    n, sw, sh, claim, claim_th = geom
    blend, canvas, with_lut = stages
    dw, dh = sw // 2, sh // 2
    reach(pbh_plan(dw, dh, n), claim, "%d x %dx%d" % (n, sw, sh))
    reach(pbh_plan(dw, dh, n, th=5), claim_th, "%d x %dx%d, PBH_TH 5" % (n, sw, sh))
    rng = np.random.default_rng(0xA17 + n + blend * 2 + canvas * 4 + with_lut * 8)
    cv = (dw + 20, dh + 12, 10, 5) if canvas else None
    cw, ch = (cv[0], cv[1]) if cv else (dw, dh)
    irow = align(sw * 4, 16) + 32
    srcs = []
    for i in range(n):
        s = rng.integers(0, 256, (sh, irow), dtype=np.uint8)
        if i % 3 == 1:
            s[:, 3::4] = 255
        elif i % 3 == 2:
            s[:, 3::4][rng.random((sh, irow // 4)) < 0.3] = 0
        srcs.append(s)
    T = Tracks(rng, srcs, cw, ch, blend=blend)
    lut = gamma_lut(rng) if with_lut else None
    wants = [oracle_chain_rgba(orc, srcs[i], sw, sh, dw, dh, 3, 1, T.l2s[i] if blend else None, T.amounts[i], lut, cv) for i in range(n)]
    prm = gpu.chain_params(sw, sh, irow, dw, dh, T.irow2, T.orow, swap_rb=1, interp=3 | PIXBUF | (0 if blend else NOBLEND), bf=0, lut=lut)
    trk = gpu.chain_tracks(T.slots(T.d_src), T.slots(T.d_l2) if blend else None, T.slots(T.d_dst))
    sws = Switches(tune)
    for aligned in (1, 0):
        for sw_ in A_SWITCHES:
            sws.set(dict(sw_, PBH_ALIGNED=aligned))
            T.reset()
            gpu.chain_amounts(prm, trk, T.slots(T.amounts) if blend else None, cv)
            for i in range(n):
                T.check(i, wants[i], "aligned %d %s" % (aligned, sw_))


# ---------------------------------------------------------------- b. lgpu_chain_yuv420p

# (tracks, sw, sh, {PBH_TH: the planner's shape}); None: no PBH_TH
B_GEOM = [(17, 260, 146, {None: dict(order=1, bands=13), 1: dict(order=1, bands=73), 2: dict(order=1, bands=37), 3: dict(order=1, bands=25), 7: dict(order=1, bands=11)}),
          (33, 512, 288, {None: dict(order=1, bands=24), 1: dict(order=2, bgroup=18, bands=144), 2: dict(order=2, bgroup=9, bands=72), 3: dict(order=1, bands=48),
                          7: dict(order=1, bands=21)}),
          (64, 1024, 576, {None: dict(order=2, bgroup=7, bands=56), 1: dict(order=2, bgroup=36, bands=288), 2: dict(order=2, bgroup=18, bands=144),
                           3: dict(order=2, bgroup=12, bands=96), 7: dict(order=2, bgroup=1, bands=42)})]
# (YVU plane order, pad, tight chroma planes, canvas, blend, LUT, q, LGPU_YUV_FIX_EDGES, out_order, swap)
B_CONFIGS = [(False, (4, 3, 1), True, True, True, True, 2, 1, 0, 1), (True, (8, 5, 7), False, False, False, False, 3, 0, 1, 0)]


@pytest.mark.parametrize("cfg", [0, 1], ids=["yuv-canvas-blend", "yvu-noblend"])
@pytest.mark.parametrize("geom", B_GEOM, ids=["17x260x146", "33x512x288", "64x1024x576"])
def test_chain_yuv420p_tracks(gpu, orc, tune, geom, cfg):
    """PBH_TH 1, 2, 3, 7 and the planner's bands: one-row bands, bands that start on odd rows; 17 tracks stay in work order 1, 33 tracks reach order 2 with one- and
    two-row bands (bgroup 18 / 9), 64 tracks run order 2 throughout, with 42 bands (bgroup 1) at PBH_TH 7.  YUV / YVU, odd chroma pitches, tight planes, a canvas,
    NOBLEND, the four table sets across the cases"""
    n, sw, sh, claims = geom
    yvu, pad, tight, canvas, blend, with_lut, q, fix, order, swap = B_CONFIGS[cfg]
    wt = (B_GEOM.index(geom) * 2 + cfg) % 4
    dw, dh = sw // 2, sh // 2
    for th, claim in claims.items():
        reach(pbh_plan(dw, dh, n, yuv=True, th=th), claim, "%d x %dx%d 4:2:0, PBH_TH %s" % (n, sw, sh, th))
    rng = np.random.default_rng(0xB17 + n * 2 + cfg)
    cv = None
    if canvas:
        nw, nh = dw + 12, dh + 10
        cv = (nw, nh, (nw - dw + 1) >> 1, (nh - dh + 1) >> 1)       # letterbox_layer's centred offsets, as orc_letterbox places the frame
        assert cv[2] % 2 == 0
    cw, ch = (cv[0], cv[1]) if cv else (dw, dh)
    srcs = [planes(rng, sw, sh, pad, tight) for _ in range(n)]
    T = Tracks(rng, srcs, cw, ch, blend=blend)
    lut = gamma_lut(rng) if with_lut else None
    ys_, us_, vs_ = srcs[0][3]
    # YVU420P: the layer's second plane is V -- the chain is handed the planes in U, V order
    stri = (ys_, vs_, us_) if yvu else (ys_, us_, vs_)
    usz, vsz = (srcs[0][2].size, srcs[0][1].size) if yvu else (srcs[0][1].size, srcs[0][2].size)
    wants = []
    for i in range(n):
        Y, A1, A2, _ = srcs[i]
        U, V = (A2, A1) if yvu else (A1, A2)
        wants.append(oracle_chain(orc, Y, U, V, stri, sw, sh, 3, order ^ swap, wt, q, fix, T.l2s[i] if blend else None, T.amounts[i], lut, cv))
    d_y = [s[0] for s in T.d_src]
    d_u, d_v = ([s[2] for s in T.d_src], [s[1] for s in T.d_src]) if yvu else ([s[1] for s in T.d_src], [s[2] for s in T.d_src])
    prm = gpu.chain_params(sw, sh, ys_, dw, dh, T.irow2, T.orow, swap_rb=swap, interp=3 | PIXBUF | (0 if blend else NOBLEND), bf=0, lut=lut)
    src = gpu.yuv_source(stri, usz, vsz, out_order=order, which_tables=wt, pb_quality=q, flags=fix)
    trk = gpu.chain_yuv_tracks(T.slots(d_y), T.slots(d_u), T.slots(d_v), T.slots(T.d_l2) if blend else None, T.slots(T.d_dst))
    for th in claims:
        tune("PBH_TH", th)
        T.reset()
        gpu.chain_yuv420p(prm, src, trk, T.slots(T.amounts) if blend else None, canvas=cv)
        for i in range(n):
            T.check(i, wants[i], "PBH_TH %s" % th)


# ---------------------------------------------------------------- c. the chain off 2:1: the ratio scalers carry its stages

# the kernel-selecting geometries of test_batch_equals_single_calls_and_the_oracle that are not the exact 2:1 (sw, sh, dw, dh, interp, switch)
C_GEOM = [(384, 216, 171, 96, 3, None), (390, 219, 130, 73, 3, None), (128, 72, 192, 108, 3, None), (128, 72, 256, 144, 3, None), (200, 120, 133, 80, 0, None),
          (384, 216, 171, 96, 3, "PB_NO_PAIRS"), (3000, 64, 100, 8, 3, None)]


@pytest.mark.parametrize("canvas", [False, True], ids=["frame", "canvas"])
@pytest.mark.parametrize("n", [17, 64])
@pytest.mark.parametrize("geom", C_GEOM, ids=["pairs", "gather", "up", "double", "nearest", "nopairs", "direct"])
def test_chain_amounts_off_half(gpu, orc, tune, geom, n, canvas):
    """lgpu_chain_amounts off 2:1: the scaler that the ratio selects (pb_scale_fused: the frame in the grid's z index) with the chain's swap / blend / LUT in its
    store, the letterbox bars as one more launch; every track against the oracle"""
    sw, sh, dw, dh, interp, switch = geom
    if switch:
        tune(switch, 1)
    rng = np.random.default_rng(0xC17 + sw + dw + n + canvas)
    cv = (dw + 11, dh + 7, 5, 3) if canvas else None
    cw, ch = (cv[0], cv[1]) if cv else (dw, dh)
    irow = align(sw * 4, 16)
    srcs = [rng.integers(0, 256, (sh, irow), dtype=np.uint8) for _ in range(n)]
    for i, s in enumerate(srcs):
        if i % 3 == 1:
            s[:, 3::4] = 255
    T = Tracks(rng, srcs, cw, ch)
    lut = gamma_lut(rng)
    prm = gpu.chain_params(sw, sh, irow, dw, dh, T.irow2, T.orow, swap_rb=1, interp=interp | PIXBUF, bf=0, lut=lut)
    gpu.chain_amounts(prm, gpu.chain_tracks(T.slots(T.d_src), T.slots(T.d_l2), T.slots(T.d_dst)), T.slots(T.amounts), cv)
    for i in range(n):
        T.check(i, oracle_chain_rgba(orc, srcs[i], sw, sh, dw, dh, interp, 1, T.l2s[i], T.amounts[i], lut, cv), "%dx%d -> %dx%d" % (sw, sh, dw, dh))


# ---------------------------------------------------------------- d. the staged walk

def test_staged_groups(gpu, orc, tune):
    """64 tracks of 200x120 -> 133x80 with the 5x5 gaussian into a 1920x1080 canvas: the staged walk, in scratch groups of 32 (the 256 MB rule: two groups),
    and with PB_CHAIN_GROUP 5 and 17 (groups that do not divide 64: 12 x 5 + 4, 3 x 17 + 13).  The tracks on either side of every group boundary (and the first
    and last) against the oracle, every other track against its own one-track call"""
    import torch
    n, sw, sh, dw, dh = 64, 200, 120, 133, 80
    cv = (1920, 1080, 893, 500)
    cw, ch = cv[0], cv[1]
    default_group = min(n, (256 << 20) // (cw * 4 * ch))
    assert default_group == 32, default_group
    rng = np.random.default_rng(0xD17)
    irow = align(sw * 4, 16)
    srcs = [rng.integers(0, 256, (sh, irow), dtype=np.uint8) for _ in range(n)]
    T = Tracks(rng, srcs, cw, ch)
    lut = gamma_lut(rng)
    prm = gpu.chain_params(sw, sh, irow, dw, dh, T.irow2, T.orow, swap_rb=1, interp=3 | PIXBUF, do_blur=1, bf=0, lut=lut)
    # every track on its own
    single = []
    for i in range(n):
        T.reset()
        gpu.chain_amounts(prm, gpu.chain_tracks([T.d_src[i]], [T.d_l2[i]], [T.d_dst[i]]), [T.amounts[i]], cv)
        single.append(T.d_dst[i].clone())
    wants = {}
    for group in (None, 5, 17):
        g = group or default_group
        edges = {0, n - 1} | {k for b in range(g, n, g) for k in (b - 1, b)}
        tune("PB_CHAIN_GROUP", group)
        T.reset()
        gpu.chain_amounts(prm, gpu.chain_tracks(T.slots(T.d_src), T.slots(T.d_l2), T.slots(T.d_dst)), T.slots(T.amounts), cv)
        torch.cuda.synchronize()
        for i in range(n):
            if i in edges:
                if i not in wants:
                    wants[i] = oracle_chain_rgba(orc, srcs[i], sw, sh, dw, dh, 3, 1, T.l2s[i], T.amounts[i], lut, cv, blur=True)
                T.check(i, wants[i], "groups of %d" % g)
            else:
                assert torch.equal(T.d_dst[i], single[i]), "groups of %d, track %d: differs from its one-track call" % (g, i)
    for i in wants:
        assert (host(single[i])[:ch, :cw * 4] == wants[i]).all(), "the one-track call of track %d" % i


# ---------------------------------------------------------------- e. the polyphase chain

def h8s_grid(dw, dh, n, spare=0):
    """launch_half8's persistent grid (resize.hip): two resident workgroups per CU, less the spare slots, at most the work list, whole groups of 8, and the XCD
    stride rule -> (grid, tiles per track)"""
    tiles_x, tiles_y = cdiv(dw, 64), cdiv(dh, 16)
    nwork = tiles_x * tiles_y * n
    grid = device_cus() * (160 * 1024 // 71904)
    if 0 < spare < grid // 2:
        grid -= spare
    grid = (min(grid, nwork) + 7) & ~7
    if grid >= 64:
        w = grid >> 3
        for k in range(6):
            if w - k < 8:
                break
            if np.gcd(w - k, tiles_x) <= 2:
                w -= k
                break
        grid = w << 3
    return grid, tiles_x * tiles_y


E_CASES = [(17, 384, 216, 192, 108, None), (64, 384, 216, 192, 108, None), (64, 384, 216, 192, 108, 24), (17, 320, 200, 200, 120, "SEP2P_FORCE"),
           (64, 320, 200, 200, 120, "SEP2P_FORCE")]


@pytest.mark.parametrize("case", E_CASES, ids=["half8s-17", "half8s-64", "half8s-64-spare", "sep2p-17", "sep2p-64"])
def test_polyphase_chain(gpu, orc, tune, case):
    """lgpu_chain (polyphase) against orc_chain.  Exact 2:1, 384x216 -> 192x108: 21 tiles per track against a persistent grid of hundreds of workgroups, and more work
    than the grid -- one stride of k_half8s' walk crosses many tracks (17 tracks: 16; 64 tracks: 24; with CHAIN_SPARE_WGS = 24 a smaller grid).  Off 2:1 with
    SEP2P_FORCE: k_sep2p's list of tiles_x * tiles_y * ntracks tiles"""
    n, sw, sh, dw, dh, switch = case
    spare = switch if isinstance(switch, int) else 0
    if switch == "SEP2P_FORCE":
        tune("SEP2P_FORCE", 1)
    elif spare:
        tune("CHAIN_SPARE_WGS", spare)
    if sw == 2 * dw:
        grid, tiles = h8s_grid(dw, dh, n, spare)
        assert tiles * n > grid and grid >= 2 * tiles, "%d tiles per track, grid %d, %d tracks: one stride must cross tracks, the list outrun the grid" % (tiles, grid, n)
    rng = np.random.default_rng(0xE17 + n + sw + (switch is not None))
    srcs = [rng.integers(0, 256, (sh, sw * 4), dtype=np.uint8) for _ in range(n)]
    T = Tracks(rng, srcs, dw, dh)
    lut = gamma_lut(rng)
    bf = 201
    prm = gpu.chain_params(sw, sh, sw * 4, dw, dh, T.irow2, T.orow, swap_rb=1, interp=3, do_blur=0, bf=bf, lut=lut)
    gpu.chain(prm, gpu.chain_tracks(T.slots(T.d_src), T.slots(T.d_l2), T.slots(T.d_dst)))
    for i in range(n):
        want = np.zeros((dh, dw * 4), np.uint8)
        assert orc.orc_chain(P(srcs[i]), sw * 4, sw, sh, P(T.l2s[i]), T.irow2, P(want), dw * 4, dw, dh, 1, 3, 0, bf, P(lut)) == 0
        T.check(i, want, "%dx%d -> %dx%d" % (sw, sh, dw, dh))


# ---------------------------------------------------------------- f. lgpu_pixbuf_scale_batch

F_GEOM = [(384, 216, 171, 96, 4, 3, None), (384, 216, 171, 96, 3, 2, None), (390, 219, 130, 73, 4, 3, None), (128, 72, 192, 108, 4, 3, None), (128, 72, 256, 144, 4, 3, None),
          (512, 64, 256, 32, 4, 3, None), (512, 64, 256, 32, 4, 2, None), (256, 64, 128, 32, 3, 3, None), (200, 120, 133, 80, 4, 0, None), (200, 120, 133, 80, 3, 0, None),
          (384, 216, 171, 96, 4, 3, "PB_NO_PAIRS"), (3000, 64, 100, 8, 4, 3, None), (64, 36, 64, 36, 4, 3, None)]


@pytest.mark.parametrize("n", [17, 64])
def test_pixbuf_scale_batch(gpu, orc, tune, n):
    """every kernel of lgpu_pixbuf_scale_batch (the geometries of test_batch_equals_single_calls_and_the_oracle) with 17 and 64 frames: translucent, opaque and
    partly transparent frames, frames handed over in a shuffled slot order, every frame against the oracle and its guard bytes"""
    rng = np.random.default_rng(0xF17 + n)
    for (sw, sh, dw, dh, ch, interp, switch) in F_GEOM:
        tune("PB_NO_PAIRS", 1 if switch else None)
        irow, orow = align(sw * ch, 16), align(dw * ch, 16) + 16
        srcs = [rng.integers(0, 256, (sh, irow), dtype=np.uint8) for _ in range(n)]
        if ch == 4:
            for k, s_ in enumerate(srcs):
                if k % 3 == 1:
                    s_[:, 3::4] = 255
                elif k % 3 == 2:
                    s_[:, 3::4][rng.random((sh, irow // 4)) < 0.4] = 0
        fills = [rng.integers(0, 256, (dh + 2, orow), dtype=np.uint8) for _ in range(n)]
        d_srcs, d_dsts = [dev(s_) for s_ in srcs], [dev(f) for f in fills]
        order = list(rng.permutation(n))
        gpu.pixbuf_scale_batch([d_srcs[i] for i in order], [d_dsts[i] for i in order], sw, sh, dw, dh, channels=ch, interp=interp)
        for i in range(n):
            want = np.zeros((dh, dw * ch), np.uint8)
            assert orc.orc_pixbuf_scale(P(srcs[i]), irow, sw, sh, P(want), dw * ch, dw, dh, ch, interp) == 0
            out = host(d_dsts[i])
            what = "%dx%d->%dx%d %dch interp %d %s: frame %d of %d" % (sw, sh, dw, dh, ch, interp, switch or "", i, n)
            assert (out[:dh, :dw * ch] == want).all(), what
            assert (out[dh:] == fills[i][dh:]).all() and (out[:dh, dw * ch:] == fills[i][:dh, dw * ch:]).all(), what + ": guard bytes written"


# ---------------------------------------------------------------- g. lgpu_yuv420p_to_rgb_batch

@pytest.fixture
def yuv_cells(gpu):
    from lives_amd import lib
    L = lib.load()
    yield lambda nc: L.lgpu_yuv420_tuning(nc, -1, -1)
    L.lgpu_yuv420_tuning(2, 512, 8)


@pytest.mark.parametrize("kernel", ["cells", "one-column"])
@pytest.mark.parametrize("is_422", [0, 1], ids=["420", "422"])
@pytest.mark.parametrize("n", [17, 64])
def test_yuv420p_to_rgb_batch(gpu, orc, yuv_cells, n, is_422, kernel):
    """the batched K2 conversion: the cell kernel (k_yuv420p_to_rgb_s, the frame in blockIdx.y) and, with lgpu_yuv420_tuning(0), the one-column kernels
    (k_yuv420p_to_rgb / k_yuv422p_to_rgb, the frame in blockIdx.z), with and without the LUT; every frame against the oracle"""
    assert yuv_cells(0 if kernel == "one-column" else 2) == 0
    rng = np.random.default_rng(0x617 + n + is_422 * 2 + (kernel == "cells"))
    w, h = 320, 180
    chh = h if is_422 else h // 2
    ys, cs, orow = w + 16, w // 2 + 8, align(w * 4, 16) + 32
    srcs = [(rng.integers(0, 256, (h, ys), dtype=np.uint8), rng.integers(0, 256, (chh, cs), dtype=np.uint8), rng.integers(0, 256, (chh, cs), dtype=np.uint8))
            for _ in range(n)]
    d_srcs = [tuple(dev(p) for p in s) for s in srcs]
    lut = gamma_lut(rng)
    for use_lut in (False, True):
        wt, order = int(rng.integers(0, 4)), int(rng.integers(0, 2))
        fills = [rng.integers(0, 256, (h + 2, orow), dtype=np.uint8) for _ in range(n)]
        d_dsts = [dev(f) for f in fills]
        slot = list(rng.permutation(n))
        gpu.yuv420p_to_rgb_batch([d_srcs[i] + (d_dsts[i],) for i in slot], w, h, out_order=order, is_422=is_422, which_tables=wt, lut=lut if use_lut else None)
        st = (ctypes.c_int * 3)(ys, cs, cs)
        for i in range(n):
            Y, U, V = srcs[i]
            want = np.zeros((h, w * 4), np.uint8)
            orc.orc_yuv420p_to_rgb(P(Y), P(U), P(V), st, U.size, V.size, P(want), w * 4, w, h, 4, order, is_422, wt, 2, P(lut) if use_lut else None, 0)
            out = host(d_dsts[i])
            what = "lut %s tables %d order %d: frame %d of %d" % (use_lut, wt, order, i, n)
            assert (out[:h, :w * 4] == want).all(), what
            assert (out[h:] == fills[i][h:]).all() and (out[:h, w * 4:] == fills[i][:h, w * 4:]).all(), what + ": guard bytes written"


# ---------------------------------------------------------------- h. 65 tracks

def test_sixty_five_tracks_are_refused(gpu):
    """every multi-track entry point: 65 tracks or frames -> LGPU_E_BADARG, nothing written; the same call with 64 runs"""
    import torch
    from lives_amd import lib
    ops, L = gpu, lib.load()
    sw, sh, dw, dh = 256, 144, 128, 72
    row = (dw + 8) * 4                  # room for the canvas form's frame
    src = torch.zeros((sh, sw * 4), dtype=torch.uint8, device="cuda")
    l2 = torch.zeros((dh, row), dtype=torch.uint8, device="cuda")
    D = torch.zeros((dh + 2, row), dtype=torch.uint8, device="cuda")
    Y = torch.zeros((sh, sw), dtype=torch.uint8, device="cuda")
    U = torch.zeros((sh // 2, sw // 2), dtype=torch.uint8, device="cuda")
    st = ops.stream_ptr()
    amounts = (ctypes.c_uint8 * 65)(*distinct_amounts(np.random.default_rng(65), 65))
    prm = ops.chain_params(sw, sh, sw * 4, dw, dh, row, row, swap_rb=1, interp=3 | PIXBUF, bf=9)
    poly = ops.chain_params(sw, sh, sw * 4, dw, dh, row, row, swap_rb=1, interp=3, bf=9)
    ysrc = ops.yuv_source((sw, sw // 2, sw // 2), U.numel(), U.numel())
    cv = lib.Canvas(dw + 8, dh, 4, 0)

    def trk(n):
        return ops.chain_tracks([src] * n, [l2] * n, [D] * n)

    def frames(n):
        f = (lib.YuvFrame * n)()
        for x in f:
            x.y_d, x.u_d, x.v_d, x.dst_d = Y.data_ptr(), U.data_ptr(), U.data_ptr(), D.data_ptr()
        return f
    calls = {
        "lgpu_chain (pixbuf)": lambda n: L.lgpu_chain(ctypes.byref(prm), trk(n), n, st),
        "lgpu_chain (polyphase)": lambda n: L.lgpu_chain(ctypes.byref(poly), trk(n), n, st),
        "lgpu_chain_canvas": lambda n: L.lgpu_chain_canvas(ctypes.byref(prm), ctypes.byref(cv), trk(n), n, st),
        "lgpu_chain_amounts": lambda n: L.lgpu_chain_amounts(ctypes.byref(prm), None, trk(n), n, amounts, st),
        "lgpu_chain_amounts with a canvas": lambda n: L.lgpu_chain_amounts(ctypes.byref(prm), ctypes.byref(cv), trk(n), n, amounts, st),
        "lgpu_chain_yuv420p": lambda n: L.lgpu_chain_yuv420p(ctypes.byref(prm), ctypes.byref(ysrc), None, ops.chain_yuv_tracks([Y] * n, [U] * n, [U] * n, [l2] * n, [D] * n),
                                                             n, amounts, st),
        "lgpu_pixbuf_scale_batch": lambda n: L.lgpu_pixbuf_scale_batch(ops.ptr_array([src] * n), ops.ptr_array([D] * n), n, sw * 4, sw, sh, row, dw, dh, 4, 3, st),
        "lgpu_yuv420p_to_rgb_batch": lambda n: L.lgpu_yuv420p_to_rgb_batch(n, frames(n), (ctypes.c_int * 3)(sw, sw // 2, sw // 2), U.numel(), U.numel(), row, dw, dh,
                                                                           4, 0, 0, 0, 2, None, 0, st),
    }
    for what, call in calls.items():
        D.fill_(0x5C)
        rc = call(65)
        torch.cuda.synchronize()
        assert rc == E_BADARG, "%s: %d, expected LGPU_E_BADARG" % (what, rc)
        assert bool((D == 0x5C).all()), "%s: the destination was written" % what
        assert call(64) == 0, "%s: 64 tracks refused (%s)" % (what, lib.last_error())
        torch.cuda.synchronize()
