"""The oracle's side of the fused chains, shared by the chain tests: the composition of the oracle's single stages that a chain launch must equal bit for bit, for a
planar 4:2:0 source (lgpu_chain_yuv420p) and for an RGBA source (lgpu_chain / lgpu_chain_amounts on the gdk-pixbuf arithmetic), and a builder for many-track launches
whose tracks all differ, so that a track that reads or writes another track's frame changes bytes."""
import ctypes

import numpy as np

from oracle import pyoracle as po
from tests.util import align, dev, host

P = po.P
BLACK = np.array([0, 0, 0, 255], np.uint8)


def planes(rng, sw, sh, pad, tight):
    """one 4:2:0 source: luma rows of sw + pad[0] bytes, chroma rows of sw / 2 + pad[1] / pad[2]; tight: each chroma plane ends with its last sample, so that K2's
    read one past the last row's end is clamped to the plane's last byte"""
    hw, hh = sw // 2, sh // 2
    ys, us, vs = sw + pad[0], hw + pad[1], hw + pad[2]
    usz = (hh - 1) * us + hw if tight else hh * us
    vsz = (hh - 1) * vs + hw if tight else hh * vs
    Y = rng.integers(0, 256, (sh, ys), dtype=np.uint8)
    U = rng.integers(0, 256, usz, dtype=np.uint8)
    V = rng.integers(0, 256, vsz, dtype=np.uint8)
    return Y, U, V, (ys, us, vs)


def oracle_chain(orc, Y, U, V, strides, sw, sh, interp, order, wt, q, fix, l2, amount, lut, canvas):
    dw, dh = sw // 2, sh // 2
    rgba = np.zeros((sh, sw * 4), np.uint8)
    st = (ctypes.c_int * 3)(*strides)
    orc.orc_yuv420p_to_rgb(P(Y), P(U), P(V), st, U.size, V.size, P(rgba), sw * 4, sw, sh, 4, order, 0, wt, q, None, fix)
    out = np.zeros((dh, dw * 4), np.uint8)
    assert orc.orc_pixbuf_scale(P(rgba), sw * 4, sw, sh, P(out), dw * 4, dw, dh, 4, interp) == 0
    w, h = dw, dh
    if canvas:
        w, h = canvas[0], canvas[1]
        big = np.zeros((h, w * 4), np.uint8)
        orc.orc_letterbox(P(out), dw * 4, dw, dh, P(big), w * 4, w, h, 4, P(BLACK))
        out = big
    if l2 is not None:
        orc.orc_blend_chroma(P(out), w * 4, P(l2), l2.strides[0], P(out), w * 4, w, h, 4, 0, amount)
    if lut is not None:
        orc.orc_gamma_apply(P(out), w * 4, w, h, 4, 0, P(lut))
    return out


def oracle_chain_rgba(orc, src, sw, sh, dw, dh, interp, swap, l2, amount, lut, canvas=None, blur=False):
    """the RGBA-source chain: [R <-> B] -> orc_pixbuf_scale -> [letterbox onto opaque black at canvas = (nwidth, nheight, offs_x, offs_y)] -> [orc_gauss5 over the
    whole canvas] -> [orc_blend_chroma with l2 at `amount`] -> [orc_gamma_apply]; l2 None: no blend (LGPU_INTERP_NOBLEND)"""
    conv = np.ascontiguousarray(src[:, :sw * 4])
    if swap:
        conv = np.zeros((sh, sw * 4), np.uint8)
        orc.orc_swizzle(po.OPS.index("swap3postalpha"), 0, P(src), src.strides[0], P(conv), sw * 4, sw, sh, None)
    out = np.zeros((dh, dw * 4), np.uint8)
    assert orc.orc_pixbuf_scale(P(conv), sw * 4, sw, sh, P(out), dw * 4, dw, dh, 4, interp) == 0
    w, h = dw, dh
    if canvas:
        w, h, ox, oy = canvas
        big = np.zeros((h, w * 4), np.uint8)
        big[:, 3::4] = 255
        big[oy:oy + dh, ox * 4:(ox + dw) * 4] = out
        out = big
    if blur:
        bl = np.zeros_like(out)
        orc.orc_gauss5(P(out), w * 4, P(bl), w * 4, w, h, 4)
        out = bl
    if l2 is not None:
        orc.orc_blend_chroma(P(out), w * 4, P(l2), l2.strides[0], P(out), w * 4, w, h, 4, 0, amount)
    if lut is not None:
        orc.orc_gamma_apply(P(out), w * 4, w, h, 4, 0, P(lut))
    return out


def distinct_amounts(rng, n):
    """n different blend amounts, 0 and 255 among them once n >= 2"""
    a = [int(v) for v in rng.permutation(254)[:n] + 1]
    if n >= 2:
        a[0], a[1] = 0, 255
    return a


class Tracks:
    """N tracks of one launch geometry, each with its own source, layer 2, blend amount and destination.  Every destination has row padding and two guard rows
    filled with its own random bytes; the device buffers are allocated in a shuffled order and handed to the launch in another (slot k carries frame order[k]),
    so that neither slot index nor address order is the frame index.

    srcs: host source frames (RGBA rows, or the (Y, U, V, strides) of planes()); l2s: host layer-2 frames (None: no blend); out: (rows, bytes) of the frame or canvas
    the chain writes into each destination."""

    GUARD = 2

    def __init__(self, rng, srcs, cw, ch, blend=True, orow=None):
        n = self.n = len(srcs)
        self.cw, self.ch = cw, ch
        self.orow = orow or align(cw * 4 + 8, 16)
        self.irow2 = align(cw * 4, 16) + 24
        self.srcs = srcs
        self.l2s = None
        if blend:
            self.l2s = [rng.integers(0, 256, (ch, self.irow2), dtype=np.uint8) for _ in range(n)]
            for a in self.l2s:
                al = a[:, 3:cw * 4:4]
                al[rng.random(al.shape) < 0.5] = 255
        self.amounts = distinct_amounts(rng, n)
        self.fills = [rng.integers(0, 256, (ch + self.GUARD, self.orow), dtype=np.uint8) for _ in range(n)]
        self.d_src, self.d_l2, self.d_dst = [None] * n, [None] * n, [None] * n
        for i in rng.permutation(n):
            s = srcs[i]
            self.d_src[i] = [dev(p) for p in s[:3]] if isinstance(s, tuple) else dev(s)
            self.d_l2[i] = dev(self.l2s[i]) if blend else None
            self.d_dst[i] = dev(self.fills[i])
        self.order = [int(k) for k in rng.permutation(n)]

    def slots(self, what):
        """a per-frame list in launch slot order"""
        return [what[k] for k in self.order]

    def reset(self):
        """the destinations back to their fill bytes (before another launch of the same tracks)"""
        for i in range(self.n):
            self.d_dst[i].copy_(dev(self.fills[i]))

    def got(self, i):
        return host(self.d_dst[i])

    def check(self, i, want, what=""):
        """frame i: the chain's bytes equal `want` and no byte outside the frame (row padding, guard rows) was written"""
        got = self.got(i)
        cw, ch = self.cw, self.ch
        bad = got[:ch, :cw * 4] != want
        assert not bad.any(), "%s frame %d: %d bytes differ from the oracle, first at %s" % (what, i, int(bad.sum()), np.argwhere(bad)[0].tolist())
        self.check_guards(i, got, what)

    def check_guards(self, i, got=None, what=""):
        got = self.got(i) if got is None else got
        cw, ch, f = self.cw, self.ch, self.fills[i]
        assert (got[:ch, cw * 4:] == f[:ch, cw * 4:]).all(), "%s frame %d: row padding was written" % (what, i)
        assert (got[ch:] == f[ch:]).all(), "%s frame %d: guard rows were written" % (what, i)
