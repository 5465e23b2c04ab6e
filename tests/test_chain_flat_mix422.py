"""lgpu_chain_flat_yuv_mix: the unscaled tick with a decoded frame of ANY of the four decoded formats on EACH layer (YUV420P, YUV422P, UYVY, YUYV) as one launch, no
RGBA frame anywhere, against the oracle's composition of the header's definition: layer 2 through the single-frame conversion of its format into a tight RGBA array
(tests/test_chain_flat_mix.py's l2_rgba for 4:2:0, tests/test_chain_flat422.py's first_stage for the 4:2:2 formats), then today's one-launch form of layer 1's format
with that array as layer 2 (tests/test_chain_flat.py's oracle_flat for 4:2:0, first_stage + oracle_tail for 4:2:2).  At size also against the device's own two
launches; and the refusals.  Bit-exact: every byte of every destination plane, and every byte of the planes' row padding and guard rows.

A pair is written (layer 1's format, layer 2's format); "A over B" in the docstrings means layer 2 = A blended over layer 1 = B.

The CPU tests show that the GPU cases cannot pass for the wrong reason, on the very frames the GPU tests draw (the case lists below are generators both sides walk):
a packed layer's answer changes when its chroma is clamped to 16..240 first (one staged table for both layers would fail), layer 2 read as the wrong format changes
the expectation, and the amounts drawn make layer 2 visible."""
import ctypes

import numpy as np
import pytest

from tests.chain_ref import distinct_amounts
from tests.offset_buffers import dev_at
from tests.test_chain_flat import SMALL, UNIT_CAP, gamma_lut, oracle_flat, plane_dims, planes_any
from tests.test_chain_flat422 import first_stage, oracle_tail, source, strides_of
from tests.test_chain_flat_mix import l2_rgba
from tests.util import align, dev, host

PIXBUF, NOBLEND = 0x100, 0x400
E_BADARG, E_UNSUPPORTED = -2, -3
RGBA, UYVY, YUYV, YUV420P, YUV422P = 0, 2, 3, 4, 5
FIX_EDGES = 1
GUARD = 2
FMTS = [RGBA, UYVY, YUYV, YUV420P]
FMT_IDS = ["rgba", "uyvy", "yuyv", "yuv420p"]
NAME = {UYVY: "uyvy", YUYV: "yuyv", YUV420P: "yuv420p", YUV422P: "yuv422p"}
KINDS = [YUV420P, YUV422P, UYVY]                                        # the three walks; YUYV is UYVY's walk under another byte order and rides in its place below
PAIRS = [(f1, f2) for f1 in KINDS for f2 in KINDS]                      # (layer 1, layer 2)


def pair_id(p):
    return "l1-%s_l2-%s" % (NAME[p[0]], NAME[p[1]])


def packed(f):
    return f in (UYVY, YUYV)


def layer(wt=0, q=2, fix=0, pad=(0, 0, 0), tight=False, yvu=False):
    """how one layer's planes are laid out and converted: table set, pb_quality, LGPU_YUV_FIX_EDGES, row padding of the planes (a packed frame's is pad[0] rounded down
    to a multiple of 4), tight chroma planes (the read one past the end is clamped), and whether the two chroma planes are drawn in the other order"""
    return dict(wt=wt, q=q, fix=fix, pad=pad, tight=tight, yvu=yvu)


def draw(rng, f, sw, sh, L):
    """one frame of format f as (planes, strides) in the order the conversion reads them: [Y, U, V] or [the packed frame]"""
    if f == YUV420P:
        Y, A1, A2, st = planes_any(rng, sw, sh, L["pad"], L["tight"])
        pl, st = [Y, A1, A2], tuple(st)
    else:
        pad = L["pad"] if f == YUV422P else (L["pad"][0] & ~3, 0, 0)
        pl = source(rng, f, sw, sh, pad, L["tight"])
        st = tuple(strides_of(f, sw, pl, pad))
    if L["yvu"] and not packed(f):
        pl, st = [pl[0], pl[2], pl[1]], (st[0], st[2], st[1])
    return pl, st


def to_rgba(orc, f, fr, sw, sh, order, L, read_as=None, is_422=1):
    """step 1 of the definition: the single-frame conversion of format f into a tight RGBA array.  read_as / is_422 = 0: the WRONG readings of the CPU tests"""
    pl, st = fr
    if f == YUV420P:
        return l2_rgba(orc, (pl[0], pl[1], pl[2], st), sw, sh, order, dict(L, yvu=False))
    return first_stage(orc, read_as or f, pl, st, sw, sh, order, L["wt"], L["q"], is_422=is_422)


def expected(orc, f1, fr1, L1, l2, sw, sh, order, swap, amount, lut, fmt, wt_sink):
    """step 2: today's one-launch form of layer 1's format with the array l2 as layer 2; the destination planes one track must equal"""
    pl, st = fr1
    if f1 == YUV420P:
        return oracle_flat(orc, pl[0], pl[1], pl[2], st, sw, sh, order, swap, L1["wt"], L1["q"], L1["fix"], l2, amount, lut, None, fmt, wt_sink)
    rgba = first_stage(orc, f1, pl, st, sw, sh, order, L1["wt"], L1["q"])
    return oracle_tail(orc, rgba, sw, sh, order, swap, l2, amount, lut, None, fmt, wt_sink)


def expected_mix(orc, f1, f2, fr1, fr2, L1, L2, sw, sh, order, swap, amount, lut, fmt, wt_sink):
    return expected(orc, f1, fr1, L1, to_rgba(orc, f2, fr2, sw, sh, order ^ swap, L2), sw, sh, order, swap, amount, lut, fmt, wt_sink)


def source_of(ops, f, fr, L, order):
    pl, st = fr
    return ops.yuv_layer_source(f, st, 0 if packed(f) else pl[1].size, 0 if packed(f) else pl[2].size, out_order=order, which_tables=L["wt"], pb_quality=L["q"],
                                flags=L["fix"])


def mid_amounts(rng, n):
    """n different blend amounts in 1..254: both layers reach the result.  0 and 255 appear only where a test says so (distinct_amounts)"""
    return [int(v) + 1 for v in rng.permutation(254)[:n]]


def case(seed, f1, f2, sw, sh, fmt=RGBA, ntracks=1, L1=None, L2=None, amounts=None, itself=False, **kw):
    """the inputs of one call, drawn from `seed` alone, so that the CPU tests see the frames the GPU tests run: keyword arguments of run()"""
    rng = np.random.default_rng(seed)
    L1, L2 = L1 or layer(), L2 or layer()
    frames = [draw(rng, f1, sw, sh, L1) for _ in range(ntracks)]
    frames2 = frames if itself else [draw(rng, f2, sw, sh, L2) for _ in range(ntracks)]
    amounts = amounts if amounts is not None else mid_amounts(rng, ntracks)
    return dict(seed=seed, f1=f1, f2=f2, sw=sw, sh=sh, fmt=fmt, ntracks=ntracks, L1=L1, L2=L2, frames=frames, frames2=frames2, amounts=amounts, itself=itself, **kw)


def up(p, off=None):
    a = p if p.ndim == 2 else p.reshape(1, -1)
    return dev(p) if off is None else dev_at(np.ascontiguousarray(a), off)


def run(gpu, orc, seed, f1, f2, sw, sh, fmt, ntracks, L1, L2, frames, frames2, amounts, itself=False, lut=None, order=0, swap=0, wt_sink=0, yvu_sink=False,
        pads=(8, 3, 5), dst_off=0, l1_offs=None, l2_offs=None, null_chroma=True):
    """one call with ntracks tracks that all differ; the device buffers are allocated in a shuffled order and handed over in another (slot order != frame order);
    every destination plane is compared whole: frame bytes against the oracle, row padding and guard rows against their fill.  dst_off: the address of the first
    destination plane modulo 64; l1_offs / l2_offs: the addresses of a layer's planes modulo 64 (None: wherever the allocator puts them); itself: layer 2's
    pointers are layer 1's; null_chroma: a packed layer's chroma pointers are NULL (else they point at the destination, which must not matter: they are not read)"""
    ops = gpu
    rng = np.random.default_rng([int(v) for v in np.atleast_1d(seed)] + [1])
    dims = plane_dims(fmt, sw, sh)
    strides = [align(b + pads[k], 4 if fmt in (RGBA, UYVY, YUYV) else 2 if k == 0 else 1) for k, (b, _) in enumerate(dims)]
    fills = [[rng.integers(0, 256, (r + GUARD, strides[k]), dtype=np.uint8) for k, (_, r) in enumerate(dims)] for _ in range(ntracks)]
    d1, d2, d_pl = [None] * ntracks, [None] * ntracks, [None] * ntracks
    for i in rng.permutation(ntracks):
        d_pl[i] = [dev_at(f, dst_off if k == 0 else 0) for k, f in enumerate(fills[i])]
        if not itself:
            d2[i] = [up(p, l2_offs[j] if l2_offs else None) for j, p in enumerate(frames2[i][0])]
        d1[i] = [up(p, l1_offs[j] if l1_offs else None) for j, p in enumerate(frames[i][0])]
        if itself:
            d2[i] = d1[i]
    slots = [int(k) for k in rng.permutation(ntracks)]
    dsel = [0, 2, 1] if (yvu_sink and fmt == YUV420P) else list(range(len(dims)))
    prm = ops.chain_params(sw, sh, 0, sw, sh, 0, strides[0] if fmt == RGBA else 0, swap_rb=swap, interp=PIXBUF, bf=0, lut=lut)
    src, src2 = source_of(ops, f1, frames[0], L1, order), source_of(ops, f2, frames2[0], L2, order ^ swap)
    sink = ops.chain_sink(fmt, [strides[j] for j in dsel], which_tables=wt_sink, in_order=order ^ swap) if fmt != RGBA else None

    def chroma(d, f, j):
        return [d[k][j] for k in slots] if not packed(f) else None
    trk = ops.chain_yuv_mix_tracks([d1[k][0] for k in slots], chroma(d1, f1, 1), chroma(d1, f1, 2), [d2[k][0] for k in slots], chroma(d2, f2, 1), chroma(d2, f2, 2),
                                   [[d_pl[k][j] for j in dsel] for k in slots])
    if not null_chroma:
        for t in trk:
            if packed(f1):
                t.u_d = t.v_d = t.dst_d[0]
            if packed(f2):
                t.u2_d = t.v2_d = t.dst_d[0]
    ops.chain_flat_yuv_mix(prm, src, src2, trk, [amounts[k] for k in slots], sink=sink)
    wants = []
    for i in range(ntracks):
        want = expected_mix(orc, f1, f2, frames[i], frames2[i], L1, L2, sw, sh, order, swap, amounts[i], lut, fmt, wt_sink)
        wants.append(want)
        for p, j in enumerate(dsel):              # p: the conversion's plane (Y, U, V); j: the buffer it was handed
            b, r = dims[p]
            got = host(d_pl[i][j])
            bad = got[:r, :b] != want[p][:r, :b]
            assert not bad.any(), "%s over %s, %dx%d fmt %d track %d plane %d: %d bytes differ from the oracle, first at %s" % (
                NAME[f2], NAME[f1], sw, sh, fmt, i, p, int(bad.sum()), np.argwhere(bad)[0].tolist())
            assert (got[:r, b:] == fills[i][j][:r, b:]).all(), "track %d plane %d: row padding was written" % (i, p)
            assert (got[r:] == fills[i][j][r:]).all(), "track %d plane %d: guard rows were written" % (i, p)
    return wants


def drawn_layer(rng, f, i):
    return layer(wt=int(rng.integers(0, 2 if packed(f) else 4)), q=int(rng.integers(1, 4)), fix=int(rng.integers(0, 2)) * FIX_EDGES,
                 pad=(int(rng.integers(0, 6)), int(rng.integers(0, 6)), 1 + 2 * i), tight=bool(rng.integers(0, 2)), yvu=bool(rng.integers(0, 2)))


# ---- the case lists: generators of run()'s keyword arguments, walked by the GPU tests and by the CPU tests of their premises ------------------------------------------
def stage_cases(pair, fmt, with_lut):
    """test 1: the two sizes x both swap_rb, two tracks with distinct amounts in 1..254; per layer and independently: tables, quality, FIX_EDGES, pitches, tight chroma
    planes, plane order; the sink's plane order and tables drawn too.  A packed layer is UYVY on the first size and YUYV on the second"""
    rng = np.random.default_rng([0x4D1, pair[0], pair[1], fmt, with_lut])
    for i, (sw, sh) in enumerate([(132, 76), (36, 21) if fmt != YUV420P else (36, 22)]):
        f1, f2 = (YUYV if i and packed(f) else f for f in pair)
        for swap in (0, 1):
            wt_sink = int(rng.integers(0, 4)) if fmt == YUV420P else int(rng.integers(0, 2))
            yield case(int(rng.integers(1 << 30)), f1, f2, sw, sh, fmt, ntracks=2, L1=drawn_layer(rng, f1, i), L2=drawn_layer(rng, f2, i), order=int(rng.integers(0, 2)), swap=swap,
                       wt_sink=wt_sink, yvu_sink=bool(rng.integers(0, 2)), pads=(8 * i, 3 + 2 * i, 7), with_lut=with_lut)


SMALL_PAIRS = [(UYVY, YUV422P), (YUV420P, UYVY), (YUV422P, YUV420P), (YUYV, YUYV), (YUV422P, UYVY), (UYVY, YUV420P), (YUV420P, YUV422P), (YUV422P, YUV422P)]
SMALL_420 = [g for g in SMALL if not g[1] & 1] + [(2, 4)]


def small_cases(pair, sw, sh, fmts):
    """test 2: tight and loose chroma planes (tight on one layer, loose on the other, then the other way round), odd pitches, FIX_EDGES on one layer"""
    f1, f2 = pair
    for t, tight in enumerate((True, False)):
        for fmt in fmts:
            out = fmt if fmt != UYVY or tight else YUYV
            yield case([0x5A3, f1, f2, sw, sh, t, fmt], f1, f2, sw, sh, out, ntracks=2, L1=layer(fix=t, q=3 - t, pad=(4 * t, 1, 3), tight=tight, wt=t),
                       L2=layer(fix=1 - t, q=1 + t, pad=(4 - 4 * t, 3, 1), tight=not tight, wt=1 - t), swap=t, order=int(fmt == UYVY), wt_sink=t, pads=(2, 1, 3) if fmt == YUV420P else (8, 3, 5))


def table_cases():
    """test 3: (what, f1, L1, f2, L2).  A packed layer beside a planar one under the same which_tables (0: the planar layer's index is clamped to 16..240 and the
    packed layer's is not, so the set is shared and the staged copy cannot be; 1: neither is clamped), both ways round; planar pairs under table sets 0/1, 0/2,
    0/3, both ways round.  Chroma samples are drawn over the whole 0..255 range (test_tables_frames_leave_the_clamp checks the frames)"""
    out = []
    for wt in (0, 1):
        for planar in (YUV420P, YUV422P):
            out.append(("uyvy over %s, both tables %d" % (NAME[planar], wt), planar, layer(wt=wt, pad=(1, 1, 3)), UYVY, layer(wt=wt, pad=(4, 0, 0))))
            out.append(("%s over uyvy, both tables %d" % (NAME[planar], wt), UYVY, layer(wt=wt), planar, layer(wt=wt, pad=(3, 1, 1))))
        out.append(("yuyv over uyvy, both tables %d" % wt, UYVY, layer(wt=wt), YUYV, layer(wt=wt, pad=(4, 0, 0))))
    for k, wt in enumerate((1, 2, 3)):
        fa, fb = [(YUV420P, YUV422P), (YUV422P, YUV422P), (YUV422P, YUV420P)][k]
        out.append(("%s tables %d over %s tables 0" % (NAME[fb], wt, NAME[fa]), fa, layer(wt=0, pad=(1, 1, 3)), fb, layer(wt=wt, pad=(3, 1, 1))))
        out.append(("%s tables 0 over %s tables %d" % (NAME[fb], NAME[fa], wt), fa, layer(wt=wt, pad=(1, 1, 3)), fb, layer(wt=0, pad=(3, 1, 1))))
    return out


TABLE_CASES = table_cases()
TABLE_IDS = [c[0].replace(" ", "_").replace(",", "") for c in TABLE_CASES]


def table_case(k, fmt):
    what, f1, L1, f2, L2 = TABLE_CASES[k]
    return case([0x7AB, k, fmt], f1, f2, 36, 22, fmt, ntracks=2, L1=L1, L2=L2, swap=k & 1)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_yuv_layer_source_struct_and_symbol():
    """lgpu_yuv_layer_source as include/lives_gpu.h lays it out (int, int[3], long, long, int x 4: 48 bytes on LP64), lgpu_yuv422_source beside it unchanged, and the
    entry point in the built library"""
    from lives_amd import lib
    S = lib.YuvLayerSource
    assert ctypes.sizeof(S) == 48 and S.in_fmt.offset == 0 and S.istrides.offset == 4 and S.u_size.offset == 16 and S.v_size.offset == 24
    assert S.out_order.offset == 32 and S.which_tables.offset == 36 and S.pb_quality.offset == 40 and S.flags.offset == 44
    assert ctypes.sizeof(lib.Yuv422Source) == 48 and ctypes.sizeof(lib.ChainYuvMixTrack) == 72
    assert "lgpu_chain_flat_yuv_mix" in lib.PROTOTYPES and len(lib.PROTOTYPES["lgpu_chain_flat_yuv_mix"]) == 8
    assert hasattr(lib.load(), "lgpu_chain_flat_yuv_mix")
    from lives_amd import ops
    s = ops.yuv_layer_source(UYVY, (264,), out_order=1, which_tables=1, pb_quality=3, flags=1)
    assert (s.in_fmt, s.istrides[0], s.istrides[1], s.u_size, s.out_order, s.which_tables, s.pb_quality, s.flags) == (2, 264, 0, 0, 1, 1, 3, 1)


@pytest.mark.parametrize("k", range(len(TABLE_CASES)), ids=TABLE_IDS)
def test_tables_frames_leave_the_clamp(orc, k):
    """on the frames test_mix422_staged_tables draws: chroma samples below 16 and above 240 exist on every layer.  With which_tables 1 a packed layer's conversion
    changes when its chroma samples are clamped to 16..240 first -- what a kernel would compute that indexed its tables through a clamp.  With which_tables 0 it does
    NOT: the reference's clamped tables are flat below 16 and from 240 up (host_tables.cpp: every chroma entry at or below 16 is 0, every one from 240 up is the
    entry of 240), so table[clamp(e)] == table[e] and the bytes cannot tell a shared staged copy from two.  The kernel stages two all the same (the rule does not lean
    on the tables' shape); the GPU case then pins the bytes, not the copy count.  For the planar table pairs, layer 2 converted with layer 1's table set differs"""
    c = table_case(k, RGBA)
    sw, sh = c["sw"], c["sh"]
    for f, fr, L in ((c["f1"], c["frames"][1], c["L1"]), (c["f2"], c["frames2"][1], c["L2"])):
        if packed(f):
            a = fr[0][0][:, :sw * 2]
            cb = a[:, (0 if f == UYVY else 1)::2]
            assert (cb < 16).any() and (cb > 240).any()
            cl = fr[0][0].copy()
            cl[:, (0 if f == UYVY else 1)::2] = np.clip(cl[:, (0 if f == UYVY else 1)::2], 16, 240)
            changed = bool((to_rgba(orc, f, fr, sw, sh, 0, L) != to_rgba(orc, f, ([cl], fr[1]), sw, sh, 0, L)).any())
            assert changed == bool(L["wt"] & 1), "which_tables %d: clamping a packed layer's chroma %s the bytes" % (L["wt"], "changed" if changed else "left")
        else:
            assert all((p < 16).any() and (p > 240).any() for p in fr[0][1:])
    if c["L1"]["wt"] != c["L2"]["wt"]:
        right = to_rgba(orc, c["f2"], c["frames2"][1], sw, sh, 0, c["L2"])
        assert (right != to_rgba(orc, c["f2"], c["frames2"][1], sw, sh, 0, dict(c["L2"], wt=c["L1"]["wt"]))).any()


def wrong_reading(orc, c, i):
    """track i's expectation, and the one with layer 2 read as the wrong format: YUV422P as 4:2:0 (is_422 = 0), UYVY as YUYV and the reverse"""
    f2, sw, sh, order, swap = c["f2"], c["sw"], c["sh"], c.get("order", 0), c.get("swap", 0)
    wrong_l2 = (to_rgba(orc, f2, c["frames2"][i], sw, sh, order ^ swap, c["L2"], is_422=0) if f2 == YUV422P else
                to_rgba(orc, f2, c["frames2"][i], sw, sh, order ^ swap, c["L2"], read_as=UYVY + YUYV - f2))
    args = (sw, sh, order, swap, c["amounts"][i], None, c["fmt"], c.get("wt_sink", 0))
    right = expected_mix(orc, c["f1"], f2, c["frames"][i], c["frames2"][i], c["L1"], c["L2"], *args)
    return right, expected(orc, c["f1"], c["frames"][i], c["L1"], wrong_l2, *args)


@pytest.mark.parametrize("pair", [p for p in PAIRS if p[1] != YUV420P], ids=pair_id)
def test_stage_frames_tell_layer2s_format(orc, pair):
    """on the frames test_mix422_stages draws (to RGBA, YUV420P and UYVY): reading layer 2 as the wrong format changes every track's expectation"""
    for fmt, with_lut in ((RGBA, False), (RGBA, True), (YUV420P, False), (UYVY, True)):
        for c in stage_cases(pair, fmt, with_lut):
            for i in range(c["ntracks"]):
                right, wrong = wrong_reading(orc, c, i)
                assert any((a != b).any() for a, b in zip(right, wrong)), "%s read wrongly gives the same bytes (%dx%d)" % (NAME[c["f2"]], c["sw"], c["sh"])


@pytest.mark.parametrize("pair", [p for p in SMALL_PAIRS if p[1] != YUV420P], ids=pair_id)
def test_small_frames_tell_layer2s_format(orc, pair):
    """on the frames test_mix422_smallest_frames draws: reading layer 2 as the wrong format changes the expectation.  A YUV422P frame of ONE row is left out: the two
    walks agree there by construction (row 0 of either reads chroma row 0 with the same neighbours) unless the read past the row's end is in play"""
    for sw, sh in SMALL:
        if pair[1] == YUV422P and sh == 1:
            continue
        differ = 0
        for c in small_cases(pair, sw, sh, [RGBA]):
            for i in range(c["ntracks"]):
                right, wrong = wrong_reading(orc, c, i)
                differ += int(any((a != b).any() for a, b in zip(right, wrong)))
        assert differ == 4, "%s %dx%d: %d of 4 expectations change when layer 2 is read wrongly" % (pair_id(pair), sw, sh, differ)


def test_amounts_make_layer2_visible(orc):
    """mid_amounts() never draws 0 or 255, and at the amounts the stage and small-frame cases draw another layer 2 changes the expectation; at amount 0 (only
    test_mix422_tracks hands it over, with 255, through distinct_amounts) layer 2 does not reach the result"""
    rng = np.random.default_rng(0xA1)
    for n in (1, 2, 64, 254):
        a = mid_amounts(rng, n)
        assert len(set(a)) == n and min(a) >= 1 and max(a) <= 254
    assert distinct_amounts(rng, 7)[:2] == [0, 255]
    for pair in ((YUV420P, UYVY), (UYVY, YUV422P), (YUV422P, YUV420P)):
        for c in list(stage_cases(pair, RGBA, False)) + list(small_cases(pair, 6, 5, [UYVY])):
            assert all(1 <= a <= 254 for a in c["amounts"])
            other = draw(np.random.default_rng(7), c["f2"], c["sw"], c["sh"], c["L2"])
            for i in range(c["ntracks"]):
                args = (c["L1"], c["L2"], c["sw"], c["sh"], c.get("order", 0), c.get("swap", 0))
                tail = (None, c["fmt"], c.get("wt_sink", 0))
                mine = expected_mix(orc, c["f1"], c["f2"], c["frames"][i], c["frames2"][i], *args, c["amounts"][i], *tail)
                theirs = expected_mix(orc, c["f1"], c["f2"], c["frames"][i], other, *args, c["amounts"][i], *tail)
                assert any((a != b).any() for a, b in zip(mine, theirs))
                none = expected_mix(orc, c["f1"], c["f2"], c["frames"][i], c["frames2"][i], *args, 0, *tail)
                assert all((a == b).all() for a, b in zip(none, expected_mix(orc, c["f1"], c["f2"], c["frames"][i], other, *args, 0, *tail)))


def go(gpu, orc, c, **more):
    c = dict(c, **more)
    lut = gamma_lut(orc) if c.pop("with_lut", False) else None
    return run(gpu, orc, lut=lut, **c)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("with_lut", [True, False], ids=["lut", "nolut"])
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("pair", PAIRS, ids=pair_id)
def test_mix422_stages(gpu, orc, pair, fmt, with_lut):
    """1. every pair to every destination (stage_cases)"""
    for c in stage_cases(pair, fmt, with_lut):
        go(gpu, orc, c)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", SMALL_PAIRS, ids=pair_id)
@pytest.mark.parametrize("sw,sh", SMALL)
def test_mix422_smallest_frames(gpu, orc, sw, sh, pair):
    """2. the walks' smallest frames to RGBA and the packed sinks: row 0 alone, with and without a row pair and the trailing row; the first pair's seed from chroma
    row i >> 1 on layer 2, the clamped read past the plane's end, chroma widths 65 and 66"""
    for c in small_cases(pair, sw, sh, [RGBA, UYVY]):
        go(gpu, orc, c, with_lut=True)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", SMALL_PAIRS, ids=pair_id)
@pytest.mark.parametrize("sw,sh", SMALL_420)
def test_mix422_smallest_frames_yuv420p(gpu, orc, sw, sh, pair):
    """2. the same to the 4:2:0 sink on the even heights of the list and 2x4"""
    for c in small_cases(pair, sw, sh, [YUV420P]):
        go(gpu, orc, c, with_lut=True)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(TABLE_CASES)), ids=TABLE_IDS)
def test_mix422_staged_tables(gpu, orc, k):
    """3. each layer converts through ITS staged tables: same set with another index clamp, other sets, both ways round (table_cases), to RGBA and to YUYV"""
    go(gpu, orc, table_case(k, RGBA))
    go(gpu, orc, table_case(k, YUYV), with_lut=True, order=1)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [RGBA, YUV420P], ids=["rgba", "yuv420p"])
@pytest.mark.parametrize("pair", [(UYVY, YUV422P), (YUV420P, YUYV)], ids=pair_id)
def test_mix422_wide_and_tall(gpu, orc, pair, fmt):
    """4. 1100 pixels: 550 cells per row, three workgroups along x with the last one partly empty; a frame of width 4 with more units than a launch's workgroup rows
    (each workgroup then walks a run of units); YUV422P over UYVY and YUYV over YUV420P"""
    f1, f2 = pair
    go(gpu, orc, case([0x71D3, f1, f2, fmt, 0], f1, f2, 1100, 10 if fmt == YUV420P else 9, fmt, L1=layer(tight=True, pad=(0, 1, 1)), L2=layer(fix=FIX_EDGES, pad=(4, 0, 3), tight=True)),
       with_lut=True)
    go(gpu, orc, case([0x71D3, f1, f2, fmt, 1], f1, f2, 4, 2 * UNIT_CAP + 6, fmt, L1=layer(fix=FIX_EDGES, pad=(4, 1, 1)), L2=layer(wt=1, pad=(0, 1, 0), tight=True), swap=1))


@pytest.mark.gpu
@pytest.mark.parametrize("dst_off", [4, 12])
def test_mix422_addresses(gpu, orc, dst_off):
    """5. a packed layer 2 at 0, 4, 8 and 12 mod 16 (and a packed layer 1 at another of them); a planar layer 2's planes at odd addresses with odd pitches; the
    destination at 4 and 12 mod 16 with pitches of 4 mod 8 (4-byte stores where the address is not a multiple of 8), 4:2:0 luma at 2 mod 4; a packed layer's unread
    chroma pointers pointing at the destination"""
    assert (132 * 4 + 4) % 8 == 4 and (132 * 2 + 4) % 8 == 4
    for n, off in enumerate((0, 4, 8, 12)):
        f1, f2 = [(YUV420P, UYVY), (YUV422P, YUYV), (YUYV, UYVY), (UYVY, YUYV)][n]
        l1_offs = (12 - off, 0, 0) if packed(f1) else (1, 3, 5)
        for fmt, pads, doff in ((RGBA, (4, 0, 0), dst_off), (UYVY, (4, 0, 0), dst_off), (YUV420P, (2, 1, 1), dst_off + 2)):
            go(gpu, orc, case([0xADF, dst_off, off, fmt], f1, f2, 132, 8, fmt, ntracks=2, L1=layer(pad=(4, 1, 1)), L2=layer(pad=(4 * (n & 1), 0, 0), wt=1)), pads=pads, dst_off=doff,
               l1_offs=l1_offs, l2_offs=(off, 0, 0), null_chroma=bool(n & 1), with_lut=fmt == RGBA)
    for f1, f2, offs in ((UYVY, YUV422P, (1, 3, 5)), (YUV422P, YUV420P, (3, 1, 7)), (YUV420P, YUV422P, (5, 7, 1))):
        for fmt, pads, doff in ((RGBA, (4, 0, 0), dst_off), (YUV420P, (2, 1, 1), dst_off + 2)):
            go(gpu, orc, case([0xADF, dst_off, f1, f2, fmt], f1, f2, 132, 8, fmt, ntracks=2, L2=layer(pad=(1, 3, 1), wt=1)), pads=pads, dst_off=doff, l2_offs=offs)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("f", [YUV422P, UYVY, YUYV, YUV420P], ids=lambda f: NAME[f])
def test_mix422_a_clip_with_itself(gpu, orc, f, fmt):
    """5. layer 2's pointers are layer 1's where the formats agree: the same planes under the same description, and under another table set and quality"""
    sh = 22 if fmt == YUV420P else 21
    L = layer(pad=(4, 1, 3))
    go(gpu, orc, case([0x5E1F, f, fmt, 0], f, f, 36, sh, fmt, ntracks=2, L1=L, L2=L, itself=True), with_lut=True)
    go(gpu, orc, case([0x5E1F, f, fmt, 1], f, f, 36, sh, fmt, L1=L, L2=dict(L, wt=1, q=1), itself=True), swap=1)


@pytest.mark.gpu
@pytest.mark.parametrize("ntracks", [1, 7, 32, 33, 64])
def test_mix422_tracks(gpu, orc, ntracks):
    """6. 1 .. 64 tracks in one call, YUV422P over UYVY, shuffled buffers and slot order, to RGBA and to YUV420P; 32 tracks per launch, so 33 and 64 go as two.  The
    amounts are distinct_amounts(): 0 and 255 are among them from two tracks on"""
    rng = np.random.default_rng(0x7AE + ntracks)
    go(gpu, orc, case([0x7AE, ntracks, 0], UYVY, YUV422P, 68, 10, RGBA, ntracks=ntracks, L1=layer(wt=1, pad=(4, 0, 0)), L2=layer(wt=2, pad=(0, 3, 1)), amounts=distinct_amounts(rng, ntracks)),
       swap=1, with_lut=True)
    go(gpu, orc, case([0x7AE, ntracks, 1], UYVY, YUV422P, 68, 10, YUV420P, ntracks=ntracks, L1=layer(), L2=layer(wt=3, pad=(2, 2, 0), yvu=True), amounts=distinct_amounts(rng, ntracks)),
       order=1, wt_sink=2, yvu_sink=True, with_lut=True)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_mix422_both_420_is_the_420_mix(gpu, orc, fmt):
    """7. in_fmt 4 on both layers: byte-identical to lgpu_chain_flat_yuv420p_mix on the same buffers (each layer under its own description), and the oracle's bytes"""
    import torch
    ops = gpu
    rng = np.random.default_rng(0x420 + fmt)
    lut = gamma_lut(orc)
    for i, (sw, sh) in enumerate([(132, 76), (36, 22)]):
        L1, L2 = drawn_layer(rng, YUV420P, i), drawn_layer(rng, YUV420P, i)
        c = case([0x420, fmt, i], YUV420P, YUV420P, sw, sh, fmt, ntracks=2, L1=L1, L2=L2)
        want = go(gpu, orc, c, swap=i, with_lut=True)
        dims = plane_dims(fmt, sw, sh)
        d1 = [[dev(p) for p in fr[0]] for fr in c["frames"]]
        d2 = [[dev(p) for p in fr[0]] for fr in c["frames2"]]
        outs = [[[torch.full((r, b), 0x5C, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(2)] for _ in range(2)]
        prm = ops.chain_params(sw, sh, 0, sw, sh, 0, dims[0][0], swap_rb=i, interp=PIXBUF, bf=0, lut=lut)
        sink = ops.chain_sink(fmt, [b for (b, _) in dims], which_tables=0, in_order=i) if fmt != RGBA else None
        (pl1, st1), (pl2, st2) = c["frames"][0], c["frames2"][0]
        trk = [ops.chain_yuv_mix_tracks([d[0] for d in d1], [d[1] for d in d1], [d[2] for d in d1], [d[0] for d in d2], [d[1] for d in d2], [d[2] for d in d2], o) for o in outs]
        ops.chain_flat_yuv_mix(prm, source_of(ops, YUV420P, c["frames"][0], L1, 0), source_of(ops, YUV420P, c["frames2"][0], L2, i), trk[0], c["amounts"], sink=sink)
        ops.chain_flat_yuv420p_mix(prm, ops.yuv_source(st1, pl1[1].size, pl1[2].size, out_order=0, which_tables=L1["wt"], pb_quality=L1["q"], flags=L1["fix"]),
                                   ops.yuv_source(st2, pl2[1].size, pl2[2].size, out_order=i, which_tables=L2["wt"], pb_quality=L2["q"], flags=L2["fix"]), trk[1], c["amounts"], sink=sink)
        torch.cuda.synchronize()
        for t in range(2):
            for p, (b, r) in enumerate(dims):
                assert torch.equal(outs[0][t][p], outs[1][t][p]), "track %d plane %d differs from lgpu_chain_flat_yuv420p_mix" % (t, p)
                assert (host(outs[0][t][p]) == want[t][p][:r, :b]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [RGBA, UYVY, YUV420P], ids=["rgba", "uyvy", "yuv420p"])
@pytest.mark.parametrize("pair", [(YUV420P, UYVY), (YUV422P, YUV422P), (UYVY, YUV420P)], ids=pair_id)
def test_mix422_at_size_matches_todays_launches(gpu, orc, pair, fmt):
    """8. 16 x 1920x1080 with blend and gamma, UYVY over YUV420P, YUV422P over YUV422P, YUV420P over UYVY: byte-identical to the device's own two launches on the same
    inputs -- lgpu_yuv_to_rgb_batch or lgpu_yuv420p_to_rgb_batch on layer 2, then lgpu_chain_flat_yuv420p[_to_yuv] or lgpu_chain_flat_yuv422 reading that frame"""
    import torch
    ops = gpu
    f1, f2 = pair
    w, h, n = 1920, 1080, 16
    lut = gamma_lut(orc)
    g = torch.Generator(device="cuda")
    g.manual_seed(0x16 + f1 * 64 + f2 * 8 + fmt)

    def clip(f):
        rnd = lambda r, b: [torch.randint(0, 256, (r, b), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
        if packed(f):
            return [rnd(h, w * 2), None, None], (w * 2,)
        ch = h // 2 if f == YUV420P else h
        return [rnd(h, w), rnd(ch, w // 2), rnd(ch, w // 2)], (w, w // 2, w // 2)
    (A, st1), (B, st2) = clip(f1), clip(f2)
    amounts = [int(x) for x in np.random.default_rng(0x16 + fmt).integers(1, 255, n)]
    dims = plane_dims(fmt, w, h)
    fused = [[torch.full((r, b), 0x5C, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
    today = [[torch.full((r, b), 0xC5, dtype=torch.uint8, device="cuda") for (b, r) in dims] for _ in range(n)]
    conv = [torch.zeros((h, w * 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    prm = ops.chain_params(w, h, w * 4, w, h, w * 4, w * 4, swap_rb=1, interp=PIXBUF, bf=0, lut=lut)
    sink = ops.chain_sink(fmt, [b for (b, _) in dims], which_tables=0, in_order=1) if fmt != RGBA else None
    size = lambda pl, k: 0 if pl[k] is None else pl[k][0].numel()
    wt1, wt2 = 0, 0 if packed(f1) or packed(f2) else 1          # a packed layer beside a planar one under the same set: two staged copies
    s1 = ops.yuv_layer_source(f1, st1, size(A, 1), size(A, 2), out_order=0, which_tables=wt1, pb_quality=2)
    s2 = ops.yuv_layer_source(f2, st2, size(B, 1), size(B, 2), out_order=1, which_tables=wt2, pb_quality=3, flags=FIX_EDGES)
    ops.chain_flat_yuv_mix(prm, s1, s2, ops.chain_yuv_mix_tracks(A[0], A[1], A[2], B[0], B[1], B[2], fused), amounts, sink=sink)
    if packed(f2):
        ops.yuv_to_rgb_batch([[f] for f in B[0]], conv, w, h, f2, 0, 1, 1, wt2)
    else:
        ops.yuv420p_to_rgb_batch(list(zip(B[0], B[1], B[2], conv)), w, h, 4, 1, int(f2 == YUV422P), wt2, 3, flags=FIX_EDGES if f2 == YUV420P else 0)
    if f1 == YUV420P:
        src = ops.yuv_source(st1, size(A, 1), size(A, 2), out_order=0, which_tables=wt1, pb_quality=2)
        if fmt == RGBA:
            ops.chain_flat_yuv420p(prm, src, ops.chain_yuv_tracks(A[0], A[1], A[2], conv, [t[0] for t in today]), amounts)
        else:
            ops.chain_flat_yuv420p_to_yuv(prm, src, sink, ops.chain_yuv_sink_tracks(A[0], A[1], A[2], conv, today), amounts)
    else:
        src = ops.yuv422_source(f1, st1, size(A, 1), size(A, 2), out_order=0, which_tables=wt1, pb_quality=2)
        ops.chain_flat_yuv422(prm, src, ops.chain_yuv_sink_tracks(A[0], A[1], A[2], conv, today), amounts, sink=sink)
    torch.cuda.synchronize()
    for i in range(n):
        for p in range(len(dims)):
            assert torch.equal(fused[i][p], today[i][p]), "track %d plane %d: %d bytes differ from today's launches" % (i, p, int((fused[i][p] != today[i][p]).sum()))
    assert not bool((fused[0][0] == 0x5C).all())


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [(YUV422P, UYVY), (YUYV, YUV420P), (YUV420P, YUV422P), (UYVY, YUYV)], ids=pair_id)
def test_mix422_refusals(gpu, pair):
    """9. every LGPU_E_BADARG and LGPU_E_UNSUPPORTED item of the entry point, one call each: the code is compared and the destinations' fill is still whole afterwards;
    the same call inside the form then runs, a packed layer's null chroma pointers included"""
    import torch
    from lives_amd import lib
    ops = gpu
    f1, f2 = pair
    w, h = 128, 72

    def planes(f, y, u, v):
        if packed(f):
            return [torch.full((h, w * 2), y, dtype=torch.uint8, device="cuda"), None, None], (w * 2, 0, 0)
        ch = h // 2 if f == YUV420P else h
        return [torch.full((h, w), y, dtype=torch.uint8, device="cuda")] + [torch.full((ch, w // 2), c, dtype=torch.uint8, device="cuda") for c in (u, v)], (w, w // 2, w // 2)
    (A, full1), (B, full2) = planes(f1, 0, 0, 0), planes(f2, 200, 90, 160)
    D = [torch.full((h + 16, w * 4 + 64), 0x5C, dtype=torch.uint8, device="cuda") for _ in range(3)]
    csize = lambda pl: 0 if pl[1] is None else pl[1].numel()
    ptr = lambda t: None if t is None else t.data_ptr()

    def call(fmt=YUV420P, sw_=w, sh_=h, dw_=None, dh_=None, interp=PIXBUF, blur=0, amounts=(9,), ntracks=1, null=None, null_plane=False, strides=full1, strides2=full2,
             usz=None, vsz=None, usz2=None, vsz2=None, order=0, order2=None, swap=0, wt_src=0, wt_src2=0, q=2, q2=2, flags=0, flags2=0, wt=0, in_order=None, orow=None, dst_off=0,
             in_place=None, no_src2=False, in_fmt=f1, in_fmt2=f2, off1=0, off2=0, chroma2=True):
        dw_, dh_ = sw_ if dw_ is None else dw_, sh_ if dh_ is None else dh_
        orow = orow if orow is not None else [w * 4 + 64] * 3
        prm = ops.chain_params(sw_, sh_, 0, dw_, dh_, 0, orow[0], swap_rb=swap, interp=interp, do_blur=blur, bf=0)
        src = ops.yuv_layer_source(in_fmt, strides, csize(A) if usz is None else usz, csize(A) if vsz is None else vsz, out_order=order, which_tables=wt_src, pb_quality=q,
                                   flags=flags)
        src2 = ops.yuv_layer_source(in_fmt2, strides2, csize(B) if usz2 is None else usz2, csize(B) if vsz2 is None else vsz2,
                                    out_order=(order ^ swap) if order2 is None else order2, which_tables=wt_src2, pb_quality=q2, flags=flags2)
        m = max(ntracks, 1)
        sink = ops.chain_sink(fmt, orow, which_tables=wt, in_order=(order ^ swap) if in_order is None else in_order) if fmt != RGBA else None
        trk = (lib.ChainYuvMixTrack * m)()
        for t in trk:
            t.y_d, t.u_d, t.v_d = ptr(A[0]) + off1, ptr(A[1]), ptr(A[2])
            t.y2_d, t.u2_d, t.v2_d = ptr(B[0]) + off2, ptr(B[1]) if chroma2 else None, ptr(B[2]) if chroma2 else None
            for k in range(3):
                t.dst_d[k] = D[k].data_ptr() + (dst_off if k == 0 else 0)
        if null is not None:
            setattr(trk[0], null, None)
        if null_plane:
            trk[0].dst_d[2 if fmt == YUV420P else 0] = None
        if in_place is not None:
            trk[0].dst_d[in_place[0]] = (A + B)[in_place[1]].data_ptr()
        if ntracks < 1:
            trk = (lib.ChainYuvMixTrack * 0)()
        if no_src2:
            return lib.load().lgpu_chain_flat_yuv_mix(ctypes.byref(prm), ctypes.byref(src), None, ctypes.byref(sink) if sink is not None else None, trk, len(trk),
                                                      (ctypes.c_uint8 * m)(*(list(amounts) * m)), ops.stream_ptr())
        return ops.chain_flat_yuv_mix(prm, src, src2, trk, list(amounts) * m if amounts is not None else None, sink=sink, check=False)

    def less(st, k, by):
        return tuple(v - by if j == k else v for j, v in enumerate(st))
    both_badarg = {
        "no PIXBUF": dict(interp=3),
        "NOBLEND": dict(interp=PIXBUF | NOBLEND),
        "NOBLEND and null amounts": dict(interp=PIXBUF | NOBLEND, amounts=None),
        "null amounts": dict(amounts=None),
        "no tracks": dict(ntracks=0),
        "65 tracks": dict(ntracks=65),
        "null src2": dict(no_src2=True),
        "in_fmt 1": dict(in_fmt=1),
        "in_fmt 6": dict(in_fmt=6),
        "src2 in_fmt 0": dict(in_fmt2=0),
        "src2 in_fmt 1": dict(in_fmt2=1),
        "src2 in_fmt 6": dict(in_fmt2=6),
        "null layer-1 frame / luma plane": dict(null="y_d"),
        "null layer-2 frame / luma plane": dict(null="y2_d"),
        "null destination plane": dict(null_plane=True),
        "out_order 2": dict(order=2, order2=0, in_order=0),
        "src2 out_order 2": dict(order2=2),
        "src2 out_order against the chain's (no swap)": dict(order=1, swap=0, order2=0),
        "src2 out_order against the chain's (swap)": dict(order=1, swap=1, order2=1),
        "source which_tables 4": dict(wt_src=4),
        "src2 which_tables 4": dict(wt_src2=4),
        "src2 which_tables -1": dict(wt_src2=-1),
        "pb_quality 0": dict(q=0),
        "pb_quality 4": dict(q=4),
        "src2 pb_quality 0": dict(q2=0),
        "src2 pb_quality 4": dict(q2=4),
        "unknown flag": dict(flags=2),
        "src2 unknown flag": dict(flags2=2),
        "first stride below the row": dict(strides=less(full1, 0, 4)),
        "src2 first stride below the row": dict(strides2=less(full2, 0, 4)),
        "odd sw": dict(sw_=127),
        "sw 0": dict(sw_=0),
        "sh 0": dict(sh_=0),
        "dw 0": dict(dw_=0),
        "destination is layer 1's frame / luma plane": dict(in_place=(0, 0)),
        "destination is layer 2's frame / luma plane": dict(in_place=(0, 3)),
    }
    both_unsupported = {
        "2:1": dict(dw_=w // 2, dh_=h // 2),
        "another width": dict(dw_=w + 2),
        "another height": dict(dh_=h - 1),
        "gaussian": dict(blur=1),
        "first plane of 2 GiB": dict(strides=(1 << 25, full1[1], full1[2])),
        "layer-2 first plane of 2 GiB": dict(strides2=(1 << 25, full2[1], full2[2])),
    }
    for n_, f, A_, full in (("", f1, A, full1), ("2", f2, B, full2)):
        who = "layer %s" % (n_ or "1")
        if packed(f):
            both_badarg.update({who + ": BT.709 tables with a packed layer": {"wt_src" + n_: 2}, who + ": BT.709 unclamped with a packed layer": {"wt_src" + n_: 3}})
            both_unsupported.update({who + ": packed rowstride % 4 == 2": {"strides" + n_: (w * 2 + 2, 0, 0)}, who + ": packed plane at 2 mod 4": {"off" + (n_ or "1"): 2}})
        else:
            base = 1 if n_ == "" else 4
            rows = h // 2 if f == YUV420P else h
            both_badarg.update({
                who + ": null U plane": dict(null="u%s_d" % n_),
                who + ": null V plane": dict(null="v%s_d" % n_),
                who + ": U stride below the width": {"strides" + n_: less(full, 1, 2)},
                who + ": V stride below the width": {"strides" + n_: less(full, 2, 2)},
                who + ": U plane one byte short": {"usz" + n_: (rows - 1) * (w // 2) + w // 2 - 1},
                who + ": V plane one byte short": {"vsz" + n_: (rows - 1) * (w // 2) + w // 2 - 1},
                who + ": destination is the U plane": dict(in_place=(0, base)),
                who + ": destination is the V plane": dict(in_place=(0, base + 1)),
            })
            if f == YUV422P:
                both_badarg[who + ": chroma plane of 4:2:0 size"] = {"vsz" + n_: (h // 2) * (w // 2)}
            both_unsupported.update({who + ": U plane of 2 GiB": {"usz" + n_: 1 << 31}, who + ": V plane of 2 GiB": {"vsz" + n_: 1 << 31}})
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
        "chroma sink plane is layer 1's frame / luma plane": dict(in_place=(1, 0)),
        "chroma sink plane is layer 2's frame / luma plane": dict(in_place=(2, 3)),
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
    assert call(fmt=UYVY, sh_=71) == 0                 # any height for the packed sinks
    torch.cuda.synchronize()
    assert not bool((D[0][:71, :w * 2] == 0x5C).all()) and bool((D[0][71:] == 0x5C).all()) and bool((D[0][:, w * 2:] == 0x5C).all()) and bool((D[1] == 0x5C).all())
    assert call(order=1, swap=1) == 0
    torch.cuda.synchronize()
    assert not bool((D[0][:h, :w] == 0x5C).all()) and not any(bool((d[:h // 2, :w // 2] == 0x5C).all()) for d in D[1:])
    for d in D:
        d.fill_(0x5C)
    rc = call(fmt=RGBA, sh_=71, amounts=(128,), chroma2=False)      # null u2_d / v2_d: a packed layer 2 does not read them, a planar one does
    torch.cuda.synchronize()
    if packed(f2):
        assert rc == 0
        assert not bool((D[0][:71, :w * 4] == 0x5C).all()) and bool((D[0][71:] == 0x5C).all()) and bool((D[0][:, w * 4:] == 0x5C).all()) and bool((D[1] == 0x5C).all())
    else:
        assert rc == E_BADARG and all(bool((d == 0x5C).all()) for d in D)
        assert call(fmt=RGBA, sh_=71, amounts=(128,)) == 0
        torch.cuda.synchronize()
        assert not bool((D[0][:71, :w * 4] == 0x5C).all()) and bool((D[0][71:] == 0x5C).all()) and bool((D[0][:, w * 4:] == 0x5C).all()) and bool((D[1] == 0x5C).all())
