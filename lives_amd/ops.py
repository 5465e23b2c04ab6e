"""Torch-tensor front end over the C ABI (device memory + streams come from PyTorch-ROCm; every pixel is
computed by liblivesgpu.so).  Frames are 2-D uint8 CUDA tensors [rows, rowstride_bytes].
"""
import ctypes

import numpy as np
import torch

from . import lib

vp = ctypes.c_void_p


def stream_ptr():
    return vp(torch.cuda.current_stream().cuda_stream)


def dptr(t, byte_offset=0):
    assert t.is_cuda and t.dtype == torch.uint8
    return vp(t.data_ptr() + byte_offset)


def lut_ptr(lut):
    """host LUT (numpy uint8[256] or None) -> pointer kept alive by the caller"""
    if lut is None:
        return None
    lut = np.ascontiguousarray(lut, dtype=np.uint8)
    assert lut.size == 256
    return lut.ctypes.data_as(vp), lut


def init(device=0):
    torch.cuda.set_device(device)
    lib.call("lgpu_init", device)


def tuning(name, value):
    """a launch-shape switch by name (lgpu_tuning_set; value < 0 or None clears it); returns the previous value (-1: unset)"""
    L = lib.load()
    old = L.lgpu_tuning_get(name.encode())
    assert L.lgpu_tuning_set(name.encode(), -1 if value is None else int(value)) == 0, lib.last_error()
    return old


def swizzle(op, src, dst, width, height, alpha_first=0, lut=None):
    lp = lut_ptr(lut)
    lib.call("lgpu_swizzle", op, alpha_first, dptr(src), src.stride(0), dptr(dst), dst.stride(0), width, height,
             lp[0] if lp else None, stream_ptr())


def gamma_apply(pix, width, height, psize, lut, alpha_first=0, x=0, y=0):
    lp = lut_ptr(lut)
    lib.call("lgpu_gamma_apply", dptr(pix), pix.stride(0), x, y, width, height, psize, alpha_first, lp[0] if lp else None,
             stream_ptr())


def alpha_premult(pix, width, height, alpha_first=0, un=0):
    lib.call("lgpu_alpha_premult", dptr(pix), pix.stride(0), width, height, alpha_first, un, stream_ptr())


def alpha_premult_yuva(planes, width, height, palette, clamped, un=0):
    """K9b: YUVA8888 (589, one packed plane) / YUVA4444P (545, four planes), in place"""
    pp, ss = _plane_tables(planes)
    lib.call("lgpu_alpha_premult_yuva", ctypes.addressof(pp), ctypes.addressof(ss), width, height, palette, int(bool(clamped)), int(bool(un)), stream_ptr())


def rgb_to_yuv411(src, dst, width, height, in_order=0, in_alpha=0, unclamped=0):
    """K4b: RGB family -> compact YUV411 rows ((width >> 2) * 6 bytes)"""
    lib.call("lgpu_rgb_to_yuv411", dptr(src), src.stride(0), width, height, in_order, in_alpha, dptr(dst), int(bool(unclamped)), stream_ptr())


def yuv411_to_rgb(src, dst, width_mp, height, out_order=0, out_alpha=0, unclamped=0):
    """K3b: compact YUV411 rows (width_mp * 6 bytes) -> RGB / BGR / ARGB"""
    lib.call("lgpu_yuv411_to_rgb", dptr(src), width_mp, height, dptr(dst), dst.stride(0), out_order, out_alpha, int(bool(unclamped)), stream_ptr())


def yuv420p_to_rgb(y, u, v, dst, width, height, opsize=4, out_order=0, is_422=0, which_tables=0, pb_quality=2, lut=None,
                   flags=0, u_size=None, v_size=None):
    strides = (ctypes.c_int * 3)(y.stride(0), u.stride(0), v.stride(0))
    lp = lut_ptr(lut)
    lib.call("lgpu_yuv420p_to_rgb", dptr(y), dptr(u), dptr(v), strides, u_size if u_size is not None else u.numel(),
             v_size if v_size is not None else v.numel(), dptr(dst), dst.stride(0), width, height, opsize, out_order, is_422,
             which_tables, pb_quality, lp[0] if lp else None, flags, stream_ptr())


def yuv420p_to_rgb_batch(frames, width, height, opsize=4, out_order=0, is_422=0, which_tables=0, pb_quality=2, lut=None, flags=0):
    """frames: list of (y, u, v, dst) device tensors sharing one geometry and rowstrides; one launch for all of them"""
    n = len(frames)
    arr = (lib.YuvFrame * n)()
    for i, (y, u, v, d) in enumerate(frames):
        arr[i].y_d, arr[i].u_d, arr[i].v_d, arr[i].dst_d = y.data_ptr(), u.data_ptr(), v.data_ptr(), d.data_ptr()
    y, u, v, d = frames[0]
    st = (ctypes.c_int * 3)(y.stride(0), u.stride(0), v.stride(0))
    lp = lut_ptr(lut)
    lib.call("lgpu_yuv420p_to_rgb_batch", n, arr, st, u.numel(), v.numel(), d.stride(0), width, height, opsize, out_order, is_422, which_tables,
             pb_quality, lp[0] if lp else None, flags, stream_ptr())


def yuv420p_to_rgb_lut16(y, u, v, dst, width, height, lut16, opsize=4, out_order=0, is_422=0, which_tables=0, pb_quality=2, flags=0):
    """lut16: device tensor of 65536 16-bit values (the reference's fused LUT16 variant)"""
    assert lut16.is_cuda and lut16.numel() == 65536 and lut16.element_size() == 2
    strides = (ctypes.c_int * 3)(y.stride(0), u.stride(0), v.stride(0))
    lib.call("lgpu_yuv420p_to_rgb_lut16", dptr(y), dptr(u), dptr(v), strides, u.numel(), v.numel(), dptr(dst), dst.stride(0), width, height,
             opsize, out_order, is_422, which_tables, pb_quality, lut16.data_ptr(), flags, stream_ptr())


def letterbox(src, dst, width, height, nwidth, nheight, psize, black):
    b = (ctypes.c_uint8 * 4)(*black)
    lib.call("lgpu_letterbox", dptr(src), src.stride(0), width, height, dptr(dst), dst.stride(0), nwidth, nheight, psize, b,
             stream_ptr())


def resize(src, dst, sw, sh, dw, dh, psize=4, interp=3, lut=None):
    lp = lut_ptr(lut)
    lib.call("lgpu_resize", dptr(src), src.stride(0), sw, sh, dptr(dst), dst.stride(0), dw, dh, psize, interp,
             lp[0] if lp else None, stream_ptr())


def resize_plan(sw, sh, dw, dh, psize=4, interp=3, irow=None, orow=None, src_bits=0, dst_bits=0, ntracks=1, mode=lib.PLAN_RESIZE):
    """lgpu_debug_resize_plan: the kernel a resize / polyphase chain of this geometry would launch, as a dict (path by name); host only, no device needed.
    irow / orow default to compact rows rounded up to 32 bytes; src_bits / dst_bits: the OR of the frames' addresses (only the low four bits count)"""
    al = lambda n: (n + 31) // 32 * 32
    q = lib.ResizePlanQuery(sw, sh, dw, dh, psize, interp, al(sw * psize) if irow is None else irow, al(dw * psize) if orow is None else orow,
                            src_bits & 15, dst_bits & 15, ntracks, mode)
    out = lib.ResizePlan()
    lib.call("lgpu_debug_resize_plan", ctypes.byref(q), ctypes.byref(out))
    d = {n: getattr(out, n) for n, _ in lib.ResizePlan._fields_}
    d["path"] = lib.PLAN_PATHS[out.path]
    return d


def gauss5_colorkey(src0, src1, dst, width, height, psize, is_bgr, delta, opac, col):
    lib.call("lgpu_gauss5_colorkey", dptr(src0), src0.stride(0), dptr(src1), src1.stride(0), dptr(dst), dst.stride(0), width, height, psize, int(is_bgr),
             float(delta), float(opac), int(col[0]), int(col[1]), int(col[2]), stream_ptr())


def pixbuf_scale(src, dst, sw, sh, dw, dh, channels=4, interp=3):
    lib.call("lgpu_pixbuf_scale", dptr(src), src.stride(0), sw, sh, dptr(dst), dst.stride(0), dw, dh, channels, interp, stream_ptr())


def pixbuf_plan(sw, sh, dw, dh, channels=4, interp=3, irow=None, orow=None, src_bits=0, dst_bits=0, nframes=1, mode=lib.PB_PLAN_SCALE):
    """lgpu_debug_pixbuf_plan: the kernel a gdk-pixbuf scale (or the fused chain's scale, mode PB_PLAN_CHAIN) of this geometry would launch, as a dict (path by
    name); host only, no device needed.  irow / orow default to compact rows rounded up to 16 bytes; src_bits / dst_bits: the OR of the frames' addresses (only
    the low four bits count); interp may carry LGPU_INTERP_OPAQUE"""
    al = lambda n: (n + 15) // 16 * 16
    q = lib.PixbufPlanQuery(sw, sh, dw, dh, channels, interp, al(sw * channels) if irow is None else irow, al(dw * channels) if orow is None else orow,
                            src_bits & 15, dst_bits & 15, nframes, mode)
    out = lib.PixbufPlan()
    lib.call("lgpu_debug_pixbuf_plan", ctypes.byref(q), ctypes.byref(out))
    d = {n: getattr(out, n) for n, _ in lib.PixbufPlan._fields_}
    d["path"] = lib.PB_PLAN_PATHS[out.path]
    return d


def ptr_array(tensors):
    """host array of device pointers (what the *_batch entry points take)"""
    return (ctypes.c_void_p * len(tensors))(*[dptr(t) for t in tensors])


def pixbuf_scale_batch(srcs, dsts, sw, sh, dw, dh, channels=4, interp=3):
    lib.call("lgpu_pixbuf_scale_batch", ptr_array(srcs), ptr_array(dsts), len(srcs), srcs[0].stride(0), sw, sh, dsts[0].stride(0), dw, dh, channels, interp, stream_ptr())


def gauss5(src, dst, width, height, psize=4):
    lib.call("lgpu_gauss5", dptr(src), src.stride(0), dptr(dst), dst.stride(0), width, height, psize, stream_ptr())


def blend_chroma(src1, src2, dst, width, height, psize, bf, alpha_first=0):
    lib.call("lgpu_blend_chroma", dptr(src1), src1.stride(0), dptr(src2), src2.stride(0), dptr(dst), dst.stride(0), width,
             height, psize, alpha_first, bf, stream_ptr())


def blend_luma(kind, src1, src2, dst, width, height, psize, pal_order, thresh):
    lib.call("lgpu_blend_luma", kind, dptr(src1), src1.stride(0), dptr(src2), src2.stride(0), dptr(dst), dst.stride(0), width,
             height, psize, pal_order, thresh, stream_ptr())


def blend_multi(kind, src1, src2, dst, width, height, is_bgr, bf):
    lib.call("lgpu_blend_multi", kind, dptr(src1), src1.stride(0), dptr(src2), src2.stride(0), dptr(dst), dst.stride(0), width,
             height, is_bgr, bf, stream_ptr())


def colorkey(src0, src1, dst, width, height, is_bgr, delta, opac, col):
    lib.call("lgpu_colorkey", dptr(src0), src0.stride(0), dptr(src1), src1.stride(0), dptr(dst), dst.stride(0), width, height,
             is_bgr, float(delta), float(opac), int(col[0]), int(col[1]), int(col[2]), stream_ptr())


def mirror(mode, src, dst, width, height, psize):
    lib.call("lgpu_mirror", mode, dptr(src), src.stride(0), dptr(dst), dst.stride(0), width, height, psize, stream_ptr())


def transition(kind, src1, src2, dst, width, height, psize, amount):
    lib.call("lgpu_transition", kind, dptr(src1), src1.stride(0), dptr(src2), src2.stride(0), dptr(dst), dst.stride(0), width, height, psize,
             float(amount), stream_ptr())


def fx_luts(kind, palette, p0=0., p1=0., p2=0.):
    """host tables of negate (0) / posterise (1, p0 = levels) / ccorrect (2, p0..p2 = r, g, b factors); returns uint8 [psize][256] or None"""
    out = np.zeros((4, 256), np.uint8)
    ps = lib.load().lgpu_fx_luts(kind, palette, float(p0), float(p1), float(p2), out.ctypes.data)
    return out[:ps].copy() if ps else None


def byte_luts(src, dst, width, height, psize, luts):
    luts = np.ascontiguousarray(luts, dtype=np.uint8)
    assert luts.shape == (psize, 256)
    lib.call("lgpu_byte_luts", dptr(src), src.stride(0), dptr(dst), dst.stride(0), width, height, psize, luts.ctypes.data, stream_ptr())


def deinterlace(src, dst, width, height, palette):
    """deinterlace.c:45-308; src is dst = in place"""
    lib.call("lgpu_deinterlace", dptr(src), src.stride(0), dptr(dst), dst.stride(0), width, height, palette, stream_ptr())


def triple_split(src1, src2, dst, width, height, is_bgr, start, sym, end, vert, bw, rgb):
    """layout_blends.c:24-113; src1 is dst = in place"""
    col = (ctypes.c_int * 3)(*[int(v) for v in rgb])
    lib.call("lgpu_triple_split", dptr(src1), src1.stride(0), dptr(src2), src2.stride(0), dptr(dst), dst.stride(0), width, height, int(bool(is_bgr)),
             float(start), int(bool(sym)), float(end), int(bool(vert)), float(bw), ctypes.addressof(col), stream_ptr())


def dissolve_mask(seed, width, height):
    """host float32 mask of the dissolve transition for an instance seed (multi_transitions.c:41-69)"""
    m = np.zeros(width * height, np.float32)
    assert lib.load().lgpu_dissolve_mask(ctypes.c_uint64(seed), width, height, m.ctypes.data) == 1
    return m


def dissolve(src1, src2, dst, width, height, psize, mask, amount):
    """mask: float32 device tensor of width * height values"""
    lib.call("lgpu_dissolve", dptr(src1), src1.stride(0), dptr(src2), src2.stride(0), dptr(dst), dst.stride(0), width, height, psize,
             mask.data_ptr(), float(amount), stream_ptr())


def slide_over(src1, src2, dst, width, height, psize, amount, direction, slide_lower=True, slide_upper=False):
    """slide_over.c:54-146; direction 1..4 as sover_init stores it"""
    lib.call("lgpu_slide_over", dptr(src1), src1.stride(0), dptr(src2), src2.stride(0), dptr(dst), dst.stride(0), width, height, psize,
             int(amount), int(direction), int(bool(slide_lower)), int(bool(slide_upper)), stream_ptr())


def _plane_tables(planes):
    n = len(planes)
    pp = (ctypes.c_void_p * 4)(*([dptr(t) for t in planes] + [None] * (4 - n)))
    ss = (ctypes.c_int * 4)(*([t.stride(0) for t in planes] + [0] * (4 - n)))
    return pp, ss


def rgb_to_yuv(src, dst_planes, width, height, in_order, in_alpha, out_fmt, out_alpha, which_tables):
    """K4 (see include/lives_gpu.h): src 2-D uint8 device tensor, dst_planes list of 2-D uint8 device tensors"""
    dp, ds = _plane_tables(dst_planes)
    lib.call("lgpu_rgb_to_yuv", dptr(src), src.stride(0), width, height, in_order, int(in_alpha), ctypes.addressof(dp), ctypes.addressof(ds),
             out_fmt, int(out_alpha), which_tables, stream_ptr())


def rgb_to_yuv_batch(srcs, dst_planes, width, height, in_order, in_alpha, out_fmt, out_alpha, which_tables):
    """lgpu_rgb_to_yuv_batch: K4 on up to 16 frames of one geometry in one launch; srcs: 2-D uint8 device tensors, dst_planes: a list of plane tensors per frame
    (strides are taken from frame 0)"""
    n = len(srcs)
    sp = (ctypes.c_void_p * n)(*[t.data_ptr() for t in srcs])
    dp = (ctypes.c_void_p * (4 * n))()
    for f in range(n):
        for k, t in enumerate(dst_planes[f]):
            dp[4 * f + k] = t.data_ptr()
    ds = (ctypes.c_int * 4)(*([t.stride(0) for t in dst_planes[0]] + [0] * (4 - len(dst_planes[0]))))
    lib.call("lgpu_rgb_to_yuv_batch", ctypes.addressof(sp), srcs[0].stride(0), width, height, in_order, int(in_alpha), ctypes.addressof(dp), ctypes.addressof(ds),
             out_fmt, int(out_alpha), which_tables, n, stream_ptr())


def rgb_to_yuv_lut16(src, dst, width, height, in_order, in_alpha, out_fmt, unclamped, lut16):
    """K4 with the 16-bit gamma LUT inline (UYVY / YUYV only); lut16: device tensor of 65536 16-bit entries"""
    assert lut16.is_cuda and lut16.numel() == 65536 and lut16.element_size() == 2
    lib.call("lgpu_rgb_to_yuv_lut16", dptr(src), src.stride(0), width, height, in_order, int(in_alpha), dptr(dst), dst.stride(0), out_fmt,
             int(bool(unclamped)), lut16.data_ptr(), stream_ptr())


def yuv_to_rgb(src_planes, dst, width, height, in_fmt, in_alpha, out_order, out_alpha, which_tables):
    sp, ss = _plane_tables(src_planes)
    lib.call("lgpu_yuv_to_rgb", ctypes.addressof(sp), ctypes.addressof(ss), width, height, in_fmt, int(in_alpha), dptr(dst), dst.stride(0),
             out_order, int(out_alpha), which_tables, stream_ptr())


def yuv_to_rgb_batch(src_planes, dsts, width, height, in_fmt, in_alpha, out_order, out_alpha, which_tables):
    """lgpu_yuv_to_rgb_batch: K3 on up to 16 frames of one geometry in one launch; src_planes: a list of plane tensors per frame (strides are taken from frame 0),
    dsts: 2-D uint8 device tensors"""
    n = len(dsts)
    sp = (ctypes.c_void_p * (4 * n))()
    for f in range(n):
        for k, t in enumerate(src_planes[f]):
            sp[4 * f + k] = t.data_ptr()
    ss = (ctypes.c_int * 4)(*([t.stride(0) for t in src_planes[0]] + [0] * (4 - len(src_planes[0]))))
    dp = (ctypes.c_void_p * n)(*[t.data_ptr() for t in dsts])
    lib.call("lgpu_yuv_to_rgb_batch", ctypes.addressof(sp), ctypes.addressof(ss), width, height, in_fmt, int(in_alpha), ctypes.addressof(dp), dsts[0].stride(0),
             out_order, int(out_alpha), which_tables, n, stream_ptr())


def yuv_switch_clamping(planes, palette, height, to_unclamped):
    pp, ss = _plane_tables(planes)
    lib.call("lgpu_yuv_switch_clamping", ctypes.addressof(pp), ctypes.addressof(ss), palette, height, int(to_unclamped), stream_ptr())


def yuv_repack(in_pal, out_pal, src_planes, dst_planes, width, height, unclamped=False, sampling=0):
    """YUV -> YUV repack (colourspace.c K5b); palettes are WEED_PALETTE_* numbers; raises LgpuError (LGPU_E_UNSUPPORTED) for pairs
    the library does not take"""
    sp, ss = _plane_tables(src_planes)
    dp, ds = _plane_tables(dst_planes)
    lib.call("lgpu_yuv_repack", in_pal, out_pal, ctypes.addressof(sp), ctypes.addressof(ss), ctypes.addressof(dp), ctypes.addressof(ds),
             width, height, int(bool(unclamped)), int(sampling), stream_ptr())


def softlight(src_planes, dst_planes, width, height, palette, unclamped):
    """planar YUV softlight (softlight.c): src_planes / dst_planes are lists of 2-D uint8 device tensors, one per plane"""
    n = len(src_planes)
    sp = (ctypes.c_void_p * 4)(*[dptr(t) for t in src_planes])
    dp = (ctypes.c_void_p * 4)(*[dptr(t) for t in dst_planes])
    ss = (ctypes.c_int * 4)(*[t.stride(0) for t in src_planes])
    ds = (ctypes.c_int * 4)(*[t.stride(0) for t in dst_planes])
    assert n in (3, 4)
    lib.call("lgpu_softlight", ctypes.addressof(sp), ctypes.addressof(ss), ctypes.addressof(dp), ctypes.addressof(ds), width, height,
             palette, int(unclamped), stream_ptr())


FX_SOFTLIGHT, FX_TRANSITION, FX_YUV411_TO_RGB, FX_GAUSS5_COLORKEY, FX_BLEND_CHROMA, FX_BLEND_LUMA, FX_BLEND_MULTI = 1, 2, 3, 4, 5, 6, 7


def fx_batch(op, ins0, outs, width, height, ins1=None, palette=0, ip=(0, 0, 0, 0), dp=(0., 0.), frame_dp0=None):
    """lgpu_fx_batch: ins0 / ins1 / outs are lists (one entry per frame) of lists of plane tensors; strides are taken from frame 0;
    frame_dp0: a value per frame in place of dp[0] (transitions: the amount)"""
    n = len(ins0)
    frames = (lib.FxFrame * n)()
    for f in range(n):
        for k, t in enumerate(ins0[f]):
            frames[f].in0[k] = dptr(t)
        for k, t in enumerate(ins1[f] if ins1 else []):
            frames[f].in1[k] = dptr(t)
        for k, t in enumerate(outs[f]):
            frames[f].out[k] = dptr(t)
    prm = lib.FxParams()
    prm.op, prm.width, prm.height, prm.palette = op, width, height, palette
    for k, t in enumerate(ins0[0]):
        prm.irow0[k] = t.stride(0)
    for k, t in enumerate(ins1[0] if ins1 else []):
        prm.irow1[k] = t.stride(0)
    for k, t in enumerate(outs[0]):
        prm.orow[k] = t.stride(0)
    for k in range(4):
        prm.ip[k] = int(ip[k]) if k < len(ip) else 0
    prm.dp[0], prm.dp[1] = float(dp[0]), float(dp[1]) if len(dp) > 1 else 0.
    if frame_dp0 is not None:
        per_frame = (ctypes.c_double * n)(*[float(v) for v in frame_dp0])
        prm.frame_dp0 = ctypes.cast(per_frame, ctypes.POINTER(ctypes.c_double))
    lib.call("lgpu_fx_batch", ctypes.byref(prm), frames, n, stream_ptr())


def edge(src, dst, width, height, palette, mode):
    lib.call("lgpu_edge", dptr(src), src.stride(0), dptr(dst), dst.stride(0), width, height, palette, mode, stream_ptr())


def comp_geometry(owidth, oheight, offs_x, offs_y, scale_x, scale_y):
    """pixel geometry of one compositor layer (compositor.c:197-212): offsets truncate, sizes round to even"""
    return (int(offs_x * float(owidth)), int(offs_y * float(oheight)),
            (int(owidth * scale_x + 1.) >> 1) << 1, (int(oheight * scale_y + 1.) >> 1) << 1)


def composite(dst, owidth, oheight, psize, layers, bgcol=(0, 0, 0), is_bgr=0, revz=0):
    """layers: list of (tensor or None, width, height, offs_x, offs_y, alpha) already scaled to their on-screen size"""
    n = len(layers)
    arr = (lib.CompLayer * max(1, n))()
    for i, (t, w, h, ox, oy, al) in enumerate(layers):
        arr[i].src_d = dptr(t) if t is not None else None
        arr[i].irow = t.stride(0) if t is not None else 0
        arr[i].width, arr[i].height, arr[i].offs_x, arr[i].offs_y, arr[i].alpha = w, h, ox, oy, float(al)
    bg = (ctypes.c_int * 3)(*[int(c) for c in bgcol])
    lib.call("lgpu_composite", dptr(dst), dst.stride(0), owidth, oheight, psize, int(is_bgr), ctypes.addressof(bg), ctypes.addressof(arr), n,
             int(revz), stream_ptr())


class Blurzoom:
    """stateful blurzoom instance (lgpu_blurzoom_*): one per filter instance and frame geometry"""

    def __init__(self, width, height, palette):
        h = ctypes.c_void_p()
        lib.call("lgpu_blurzoom_create", width, height, palette, ctypes.addressof(h))
        self.h = h

    def process(self, src, dst, mode=0, pattern=0):
        lib.call("lgpu_blurzoom_process", self.h, dptr(src), src.stride(0), dptr(dst), dst.stride(0), mode, pattern, stream_ptr())

    def close(self):
        if self.h:
            lib.load().lgpu_blurzoom_destroy(self.h)
            self.h = None


class RgbDelay:
    """stateful RGBdelay / YUVdelay instance (lgpu_rgbdelay_*): the frame ring lives in HBM inside the handle"""

    def __init__(self):
        h = ctypes.c_void_p()
        lib.call("lgpu_rgbdelay_create", ctypes.addressof(h))
        self.h = h

    def process(self, src, dst, width, height, palette, maxcache, on, strength, yuv_clamped=False):
        on = np.ascontiguousarray(on, dtype=np.int32)
        strength = np.ascontiguousarray(strength, dtype=np.float64)
        assert on.size == 153 and strength.size == 51
        lib.call("lgpu_rgbdelay_process", self.h, dptr(src), src.stride(0), dptr(dst), dst.stride(0), width, height, palette, int(bool(yuv_clamped)),
                 int(maxcache), on.ctypes.data, strength.ctypes.data, stream_ptr())

    def close(self):
        if self.h:
            lib.load().lgpu_rgbdelay_destroy(self.h)
            self.h = None


def _amounts(amounts, ntracks):
    """a blend amount per track as the c_uint8[] the chain_* entry points take; None (with LGPU_INTERP_NOBLEND, 0x400, in params.interp) stays None"""
    return (ctypes.c_uint8 * max(1, ntracks))(*[int(a) & 0xFF for a in amounts]) if amounts is not None else None


def _ref(struct):
    """byref of an optional argument struct (canvas, sink); None is the null pointer"""
    return ctypes.byref(struct) if struct is not None else None


def _call(name, args, check):
    """check=False returns the library's code instead of raising (tests of the refusals)"""
    return lib.call(name, *args) if check else getattr(lib.load(), name)(*args)


def chain_params(sw, sh, irow, dw, dh, irow2, orow, swap_rb=1, interp=3, do_blur=0, bf=128, lut=None, param_block=None):
    p = lib.ChainParams()
    p.param_block_d = param_block.data_ptr() if param_block is not None else None
    p.sw, p.sh, p.irow, p.dw, p.dh, p.irow2, p.orow = sw, sh, irow, dw, dh, irow2, orow
    p.swap_rb, p.interp, p.do_blur, p.bf = swap_rb, interp, do_blur, bf
    p.use_lut = 1 if lut is not None else 0
    if lut is not None:
        ctypes.memmove(p.lut8, np.ascontiguousarray(lut, dtype=np.uint8).ctypes.data, 256)
    return p


def chain_tracks(srcs, layer2s, dsts):
    n = len(srcs)
    arr = (lib.ChainTrack * n)()
    for i in range(n):
        arr[i].src_d, arr[i].layer2_d, arr[i].dst_d = srcs[i].data_ptr(), (layer2s[i].data_ptr() if layer2s is not None else None), dsts[i].data_ptr()
    return arr


def chain(params, tracks):
    lib.call("lgpu_chain", ctypes.byref(params), tracks, len(tracks), stream_ptr())


def chain_canvas(params, tracks, nwidth, nheight, offs_x, offs_y):
    cv = lib.Canvas(nwidth, nheight, offs_x, offs_y)
    lib.call("lgpu_chain_canvas", ctypes.byref(params), ctypes.byref(cv), tracks, len(tracks), stream_ptr())


def chain_amounts(params, tracks, amounts, canvas=None):
    """lgpu_chain_amounts: the chain with a blend amount per track; canvas = (nwidth, nheight, offs_x, offs_y) or None"""
    am = _amounts(amounts, len(tracks))
    cv = lib.Canvas(*canvas) if canvas is not None else None
    lib.call("lgpu_chain_amounts", ctypes.byref(params), _ref(cv), tracks, len(tracks), am, stream_ptr())


def chain_yuv_tracks(ys, us, vs, layer2s, dsts):
    """lgpu_chain_yuv_track[]: the planes of each track's 4:2:0 source (pass u / v swapped for YVU420P), layer 2 (None: LGPU_INTERP_NOBLEND) and destination"""
    n = len(ys)
    arr = (lib.ChainYuvTrack * n)()
    for i in range(n):
        arr[i].y_d, arr[i].u_d, arr[i].v_d = ys[i].data_ptr(), us[i].data_ptr(), vs[i].data_ptr()
        arr[i].layer2_d, arr[i].dst_d = (layer2s[i].data_ptr() if layer2s is not None else None), dsts[i].data_ptr()
    return arr


def yuv_source(istrides, u_size, v_size, out_order=0, which_tables=0, pb_quality=2, flags=0):
    """lgpu_yuv_source"""
    s = lib.YuvSource()
    s.istrides[0], s.istrides[1], s.istrides[2] = istrides
    s.u_size, s.v_size, s.out_order, s.which_tables, s.pb_quality, s.flags = u_size, v_size, out_order, which_tables, pb_quality, flags
    return s


def chain_yuv420p(params, src, tracks, amounts, canvas=None, check=True):
    """lgpu_chain_yuv420p: the chain of lgpu_chain_amounts starting at 4:2:0 frames, one launch; canvas = (nwidth, nheight, offs_x, offs_y) or None.
    check=False returns the library's code instead of raising (tests of the refusals)"""
    am = _amounts(amounts, len(tracks))
    cv = lib.Canvas(*canvas) if canvas is not None else None
    args = (ctypes.byref(params), ctypes.byref(src), _ref(cv), tracks, len(tracks), am, stream_ptr())
    return _call("lgpu_chain_yuv420p", args, check)


def chain_sink(out_fmt, orow, which_tables=0, in_order=0):
    """lgpu_chain_sink: out_fmt 2 UYVY / 3 YUYV / 4 YUV420P, orow = the rowstrides of the sink's planes (one or three)"""
    s = lib.ChainSink()
    s.out_fmt, s.which_tables, s.in_order = out_fmt, which_tables, in_order
    for k, v in enumerate(orow):
        s.orow[k] = int(v)
    return s


def chain_sink_tracks(srcs, layer2s, dst_planes):
    """lgpu_chain_sink_track[]: source, layer 2 (None: LGPU_INTERP_NOBLEND) and the sink's planes of each track (one tensor for UYVY / YUYV; Y, U, V for YUV420P --
    pass the chroma planes swapped for YVU420P)"""
    n = len(srcs)
    arr = (lib.ChainSinkTrack * n)()
    for i in range(n):
        arr[i].src_d, arr[i].layer2_d = srcs[i].data_ptr(), (layer2s[i].data_ptr() if layer2s is not None else None)
        for k, t in enumerate(dst_planes[i]):
            arr[i].dst_d[k] = t.data_ptr()
    return arr


def chain_to_yuv(params, sink, tracks, amounts, check=True):
    """lgpu_chain_to_yuv: the chain of lgpu_chain_amounts ending at a YUV sink, one launch and no RGBA frame.  check=False returns the library's code instead of
    raising (tests of the refusals)"""
    am = _amounts(amounts, len(tracks))
    args = (ctypes.byref(params), ctypes.byref(sink), tracks, len(tracks), am, stream_ptr())
    return _call("lgpu_chain_to_yuv", args, check)


def chain_yuv_sink_tracks(ys, us, vs, layer2s, dst_planes):
    """lgpu_chain_yuv_sink_track[]: the planes of each track's 4:2:0 source (u / v swapped for YVU420P), layer 2 (None: LGPU_INTERP_NOBLEND) and the sink's planes
    (one tensor for UYVY / YUYV; Y, U, V for YUV420P -- the chroma planes swapped for YVU420P)"""
    n = len(ys)
    arr = (lib.ChainYuvSinkTrack * n)()
    for i in range(n):
        arr[i].y_d = ys[i].data_ptr()
        arr[i].u_d, arr[i].v_d = (us[i].data_ptr(), vs[i].data_ptr()) if us is not None else (None, None)      # None: a packed frame (lgpu_chain_flat_yuv422)
        arr[i].layer2_d = layer2s[i].data_ptr() if layer2s is not None else None
        for k, t in enumerate(dst_planes[i]):
            arr[i].dst_d[k] = t.data_ptr()
    return arr


def chain_yuv420p_to_yuv(params, src, sink, tracks, amounts, check=True):
    """lgpu_chain_yuv420p_to_yuv: the chain of lgpu_chain_amounts from 4:2:0 frames to a YUV sink, one launch and no RGBA frame at either end.  check=False returns
    the library's code instead of raising (tests of the refusals)"""
    am = _amounts(amounts, len(tracks))
    args = (ctypes.byref(params), ctypes.byref(src), ctypes.byref(sink), tracks, len(tracks), am, stream_ptr())
    return _call("lgpu_chain_yuv420p_to_yuv", args, check)


def chain_flat_yuv420p(params, src, tracks, amounts, canvas=None, check=True):
    """lgpu_chain_flat_yuv420p: lgpu_yuv420p_to_rgb + lgpu_chain_amounts on frames that keep their size (sw == dw, sh == dh), one launch and no converted frame;
    arguments as chain_yuv420p.  check=False returns the library's code instead of raising (tests of the refusals)"""
    am = _amounts(amounts, len(tracks))
    cv = lib.Canvas(*canvas) if canvas is not None else None
    args = (ctypes.byref(params), ctypes.byref(src), _ref(cv), tracks, len(tracks), am, stream_ptr())
    return _call("lgpu_chain_flat_yuv420p", args, check)


def chain_flat_yuv420p_to_yuv(params, src, sink, tracks, amounts, check=True):
    """lgpu_chain_flat_yuv420p_to_yuv: the same frames to a YUV sink (UYVY / YUYV / YUV420P), one launch and no RGBA frame at either end; arguments as
    chain_yuv420p_to_yuv.  check=False returns the library's code instead of raising (tests of the refusals)"""
    am = _amounts(amounts, len(tracks))
    args = (ctypes.byref(params), ctypes.byref(src), ctypes.byref(sink), tracks, len(tracks), am, stream_ptr())
    return _call("lgpu_chain_flat_yuv420p_to_yuv", args, check)


def yuv422_source(in_fmt, istrides, u_size=0, v_size=0, out_order=0, which_tables=0, pb_quality=2):
    """lgpu_yuv422_source: in_fmt 5 YUV422P (three rowstrides, the chroma planes' sizes) / 2 UYVY / 3 YUYV (one rowstride)"""
    s = lib.Yuv422Source()
    s.in_fmt = in_fmt
    for k, v in enumerate(istrides):
        s.istrides[k] = int(v)
    s.u_size, s.v_size, s.out_order, s.which_tables, s.pb_quality = u_size, v_size, out_order, which_tables, pb_quality
    return s


def chain_flat_yuv422(params, src, tracks, amounts, sink=None, canvas=None, check=True):
    """lgpu_chain_flat_yuv422: the unscaled tick from YUV422P / UYVY / YUYV frames, one launch and no converted frame, to RGBA (sink=None, rowstride params.orow,
    optionally into canvas = (nwidth, nheight, offs_x, offs_y)) or to a YUV sink.  tracks: chain_yuv_sink_tracks (a packed frame is the y plane; u / v None).
    check=False returns the library's code instead of raising (tests of the refusals)"""
    am = _amounts(amounts, len(tracks))
    cv = lib.Canvas(*canvas) if canvas is not None else None
    args = (ctypes.byref(params), ctypes.byref(src), _ref(cv), _ref(sink), tracks, len(tracks), am, stream_ptr())
    return _call("lgpu_chain_flat_yuv422", args, check)


def chain_yuv_mix_tracks(ys, us, vs, y2s, u2s, v2s, dst_planes):
    """lgpu_chain_yuv_mix_track[]: the planes of each track's two layers (u / v swapped for YVU, per layer; None for both: a packed frame, which is the y plane --
    lgpu_chain_flat_yuv_mix) and its destination planes (one tensor for RGBA / UYVY / YUYV; Y, U, V for YUV420P -- the chroma planes swapped for YVU420P)"""
    n = len(ys)
    arr = (lib.ChainYuvMixTrack * n)()
    for i in range(n):
        arr[i].y_d, arr[i].y2_d = ys[i].data_ptr(), y2s[i].data_ptr()
        arr[i].u_d, arr[i].v_d = (us[i].data_ptr(), vs[i].data_ptr()) if us is not None else (None, None)
        arr[i].u2_d, arr[i].v2_d = (u2s[i].data_ptr(), v2s[i].data_ptr()) if u2s is not None else (None, None)
        for k, t in enumerate(dst_planes[i]):
            arr[i].dst_d[k] = t.data_ptr()
    return arr


def chain_flat_yuv420p_mix(params, src, src2, tracks, amounts, sink=None, check=True):
    """lgpu_chain_flat_yuv420p_mix: two decoded 4:2:0 frames of the project's size mixed in one launch, to RGBA (sink=None, rowstride params.orow) or to a YUV sink; no
    RGBA frame anywhere.  src2 describes layer 2 (its out_order is src.out_order ^ params.swap_rb).  check=False returns the library's code instead of raising (tests
    of the refusals)"""
    am = _amounts(amounts, len(tracks))
    args = (ctypes.byref(params), ctypes.byref(src), ctypes.byref(src2), _ref(sink), tracks, len(tracks), am, stream_ptr())
    return _call("lgpu_chain_flat_yuv420p_mix", args, check)


def yuv_layer_source(in_fmt, istrides, u_size=0, v_size=0, out_order=0, which_tables=0, pb_quality=2, flags=0):
    """lgpu_yuv_layer_source: in_fmt 4 YUV420P / 5 YUV422P (three rowstrides, the chroma planes' sizes) / 2 UYVY / 3 YUYV (one rowstride)"""
    s = lib.YuvLayerSource()
    s.in_fmt = in_fmt
    for k, v in enumerate(istrides):
        s.istrides[k] = int(v)
    s.u_size, s.v_size, s.out_order, s.which_tables, s.pb_quality, s.flags = u_size, v_size, out_order, which_tables, pb_quality, flags
    return s


def chain_flat_yuv_mix(params, src, src2, tracks, amounts, sink=None, check=True):
    """lgpu_chain_flat_yuv_mix: two decoded frames of the project's size, each YUV420P, YUV422P, UYVY or YUYV, mixed in one launch, to RGBA (sink=None, rowstride
    params.orow) or to a YUV sink; no RGBA frame anywhere.  src / src2: yuv_layer_source (src2.out_order is src.out_order ^ params.swap_rb); tracks:
    chain_yuv_mix_tracks (a packed frame is the y plane; u / v None).  check=False returns the library's code instead of raising (tests of the refusals)"""
    am = _amounts(amounts, len(tracks))
    args = (ctypes.byref(params), ctypes.byref(src), ctypes.byref(src2), _ref(sink), tracks, len(tracks), am, stream_ptr())
    return _call("lgpu_chain_flat_yuv_mix", args, check)


def chain_flat_yuv_mix_canvas(params, src, src2, tracks, amounts, canvas=None, check=True):
    """lgpu_chain_flat_yuv_mix_canvas: chain_flat_yuv_mix to RGBA with both layers letterboxed onto one canvas = (nwidth, nheight, offs_x, offs_y) of opaque black, the
    bars written by the same launch (rowstride params.orow, canvas-sized).  canvas=None: the bytes of chain_flat_yuv_mix without a sink.  check=False returns the
    library's code instead of raising (tests of the refusals)"""
    am = _amounts(amounts, len(tracks))
    cv = lib.Canvas(*canvas) if canvas is not None else None
    args = (ctypes.byref(params), ctypes.byref(src), ctypes.byref(src2), _ref(cv), tracks, len(tracks), am, stream_ptr())
    return _call("lgpu_chain_flat_yuv_mix_canvas", args, check)


def select(kind, amounts, masks=None):
    """lgpu_select: kind 0 iris rectangle / 1 iris circle / 3 dissolve, one amount (0..1) per track and, for the dissolve, one device tensor of (canvas or frame) width *
    height floats per track.  The arrays it points to are kept alive on the returned struct"""
    n = max(1, len(amounts) if amounts is not None else 0)
    s = lib.Select()
    s.kind = kind
    s._amounts = (ctypes.c_double * n)(*[float(a) for a in amounts]) if amounts is not None else None
    s.amounts = ctypes.cast(s._amounts, ctypes.POINTER(ctypes.c_double)) if s._amounts is not None else None
    s._masks = (ctypes.c_void_p * max(1, len(masks)))(*[m if m is None or isinstance(m, int) else m.data_ptr() for m in masks]) if masks is not None else None
    s.mask_d = ctypes.cast(s._masks, ctypes.POINTER(ctypes.c_void_p)) if s._masks is not None else None
    return s


def chain_flat_yuv_select(params, src, src2, tracks, kind, amounts, masks=None, sink=None, canvas=None, check=True):
    """lgpu_chain_flat_yuv_select (include/lives_gpu_select.h): two decoded frames of the project's size, each YUV420P, YUV422P, UYVY or YUYV, through a select transition
    -- kind 0 iris rectangle, 1 iris circle, 3 dissolve (masks: a device tensor of floats per track) -- in one launch that converts only the layer a pixel shows; to
    RGBA (sink=None, rowstride params.orow; canvas = (nwidth, nheight, offs_x, offs_y) letterboxes both layers and the figure is the canvas's) or to a YUV sink.  src /
    src2: yuv_layer_source; tracks: chain_yuv_mix_tracks; amounts: 0..1 per track.  check=False returns the library's code instead of raising (tests of the refusals)"""
    sel = select(kind, amounts, masks)
    cv = lib.Canvas(*canvas) if canvas is not None else None
    args = (ctypes.byref(params), ctypes.byref(src), ctypes.byref(src2), ctypes.byref(sel), _ref(cv), _ref(sink), tracks, len(tracks), stream_ptr())
    return _call("lgpu_chain_flat_yuv_select", args, check)


def luma_key(type, thresholds):
    """lgpu_luma_key: type 1 luma overlay / 2 underlay / 3 negative overlay / 4 averaged overlay (== 1) and one threshold (0..255) per track.  The array it points to
    is kept alive on the returned struct"""
    k = lib.LumaKey()
    k.type = type
    k._thresholds = (ctypes.c_uint8 * max(1, len(thresholds)))(*[int(t) for t in thresholds]) if thresholds is not None else None
    k.thresholds = ctypes.cast(k._thresholds, ctypes.POINTER(ctypes.c_uint8)) if k._thresholds is not None else None
    return k


def chain_flat_yuv_luma(params, src, src2, tracks, type, thresholds, sink=None, canvas=None, check=True):
    """lgpu_chain_flat_yuv_luma (include/lives_gpu_luma.h): two decoded frames of the project's size, each YUV420P, YUV422P, UYVY or YUYV, through a luma overlay -- type 1
    overlay, 2 underlay, 3 negative overlay, 4 averaged overlay -- in one launch that converts the keyed layer everywhere and the other layer only where it is shown;
    to RGBA (sink=None, rowstride params.orow; canvas = (nwidth, nheight, offs_x, offs_y) letterboxes both layers) or to a YUV sink.  src / src2: yuv_layer_source;
    tracks: chain_yuv_mix_tracks; thresholds: 0..255 per track.  check=False returns the library's code instead of raising (tests of the refusals)"""
    key = luma_key(type, thresholds)
    cv = lib.Canvas(*canvas) if canvas is not None else None
    args = (ctypes.byref(params), ctypes.byref(src), ctypes.byref(src2), ctypes.byref(key), _ref(cv), _ref(sink), tracks, len(tracks), stream_ptr())
    return _call("lgpu_chain_flat_yuv_luma", args, check)


def stream_probe(params, tracks, reps):
    """lgpu_debug_stream_probe: the chain's algorithmic bytes as a bare stream on the same frames, ms for `reps` launches (destinations left dirty)"""
    ms = ctypes.c_float()
    lib.call("lgpu_debug_stream_probe", ctypes.byref(params), tracks, len(tracks), reps, ctypes.byref(ms), stream_ptr())
    return ms.value


def chain_timed(params, tracks, reps):
    ms = ctypes.c_float()
    lib.call("lgpu_chain_timed", ctypes.byref(params), tracks, len(tracks), reps, ctypes.byref(ms), stream_ptr())
    return ms.value
