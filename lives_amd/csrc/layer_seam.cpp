// layer_seam.cpp -- the weed_layer_t seam (include/lives_gpu_layer.h): host-side logic of
//   convert_layer_palette_full   src/colourspace.c:12190-13928
//   gamma_convert_sub_layer      src/colourspace.c:14069-14143
//   alpha_premult                src/colourspace.c:11968-12105
//   resize_layer_full            src/colourspace.c:14759-15328
//   letterbox_layer              src/colourspace.c:15343-15567
//   create_empty_pixel_data      src/colourspace.c:11434-11700
//   calc_rowstrides              src/colourspace.c:11252-11366
//   weed_layer_clear_pixel_data  src/colourspace.c:11229-11244
//   compact_rowstrides           src/colourspace.c:14439-14496
//   unletterbox_layer            src/colourspace.c:15570-15628
// re-written around the frame-level C ABI (lives_gpu.h).  All pixel work happens in the HIP kernels; this
// file only reads / writes leaves through the accessors the host bound, moves planes over PCIe and keeps the
// reference's bookkeeping (palette, size, rowstrides, gamma, premult flag, YUV leaves, failure = untouched layer).
//
// This file holds the seam BODIES and the planner's queries.  The host's plants (leaf accessors, Layer, new host planes) are seam_weed.{h,cpp}; the device copies
// of pinned planes, the per-thread streams and struct Work are seam_resident.{h,cpp}; deferred programs are seam_lazy.{h,cpp}.
// Data movement (struct Work, seam_resident.h): an ordinary layer's planes are uploaded into per-thread scratch, the kernels run,
// the results are downloaded into freshly allocated host planes and the call synchronises ONCE before it returns (host
// bytes must be valid then).  A pinned layer (lives_gpu_layer_pin) keeps its planes in HBM: the kernels read and write
// the resident buffers directly, new planes are pool buffers registered under the new host pointer, nothing is copied and
// nothing synchronises -- the calls of a chain only enqueue work, the one synchronisation is lives_gpu_layer_sync().
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include "seam_lazy.h"

using namespace seam;
namespace {

int rgb_swizzle_op(int inpl, int outpl, int *alpha_first_arg) {
  // the selector tree of src/colourspace.c:12370-12556
  const bool swap = pal_red_first(inpl) != pal_red_first(outpl);
  *alpha_first_arg = 0;
  if (!pal_alpha_first(inpl)) {
    if (!pal_alpha_last(inpl)) {                        // RGB24 / BGR24 in
      if (!pal_alpha_first(outpl)) {
        if (!pal_alpha_last(outpl)) return LGPU_SWAP3;
        return swap ? LGPU_SWAP3ADDPOST : LGPU_ADDPOST;
      }
      return swap ? LGPU_SWAP3ADDPRE : LGPU_ADDPRE;     // -> ARGB
    }
    if (!pal_alpha_first(outpl)) {                      // RGBA / BGRA in
      if (!pal_alpha_last(outpl)) return swap ? LGPU_SWAP3DELPOST : LGPU_DELPOST;
      return LGPU_SWAP3POSTALPHA;
    }
    return swap ? LGPU_SWAP4 : LGPU_SWAPPREPOST;        // -> ARGB (alpha_first = FALSE)
  }
  *alpha_first_arg = 1;                                 // ARGB in
  if (!pal_alpha_first(outpl)) {
    if (!pal_alpha_last(outpl)) return swap ? LGPU_SWAP3DELPRE : LGPU_DELPRE;
    return swap ? LGPU_SWAP4 : LGPU_SWAPPREPOST;
  }
  return LGPU_SWAP3PREALPHA;
}

// K5 on a layer: switch_yuv_clamping_and_subspace (:10929-11090), in place on the layer's own planes
bool switch_layer_clamping(weed_plant_t *layer, const Layer &l, int oclamping) {
  Work w;
  uint8_t *d[4] = {nullptr, nullptr, nullptr, nullptr};
  int rs[4] = {0, 0, 0, 0};
  for (int p = 0; p < l.nplanes; p++) {
    d[p] = w.inout(l.pd[p], (size_t)l.rs[p] * plane_rows(l.pal, l.height, p), p == 0 ? 0 : p + 3);
    rs[p] = l.rs[p];
  }
  if (!w.ok || lgpu_yuv_switch_clamping(d, rs, l.pal, l.height, oclamping == WEED_YUV_CLAMPING_UNCLAMPED, S()) != LGPU_OK) return false;
  if (!w.finish()) return false;
  set_int(layer, WEED_LEAF_YUV_CLAMPING, oclamping);
  return true;
}


// K4b on a layer (:12627-12632 and the same case under each RGB input): width leaf becomes width >> 2 macropixels, the new frame is
// written as compact macropixel rows whatever rowstride it was given (the reference passes none).  `flags` = host_flags after the
// reference's premultiplied-alpha bookkeeping (:12290-12306), done by the caller for every palette pair.
lives_gpu_boolean rgb_layer_to_yuv411(weed_plant_t *layer, const Layer &l, int oclamping, int flags) {
  const int order = pal_order(l.pal);
  const int in_alpha = pal_has_alpha(l.pal) ? 1 : 0, wm = l.width >> 2;
  if (wm < 1 || l.height < 1) return decline(layer);
  NewPlanes np;
  if (!alloc_planes(WEED_PALETTE_YUV411, wm, l.height, 0, &np)) return 0;
  Work w;
  const uint8_t *d_in = w.in(l.pd[0], (size_t)l.rs[0] * l.height, 0);
  uint8_t *d_out = w.out(np.pd[0], np.sz[0], 3, true);
  const bool ok = w.ok && lgpu_rgb_to_yuv411(d_in, l.rs[0], l.width, l.height, order, in_alpha, d_out, oclamping == WEED_YUV_CLAMPING_UNCLAMPED, S()) == LGPU_OK &&
                  w.finish();
  if (!ok) { drop_new_planes(np); return 0; }
  free_planes(l);
  commit_planes(layer, WEED_PALETTE_YUV411, wm, l.height, np);
  if (flags != l.flags) set_int(layer, kLeafHostFlags, flags);
  set_int(layer, WEED_LEAF_YUV_CLAMPING, oclamping);                         // conv_done, as for the other RGB -> YUV cases below
  set_int(layer, WEED_LEAF_YUV_SUBSPACE, l.gamma == WEED_GAMMA_BT709 ? WEED_YUV_SUBSPACE_BT709 : WEED_YUV_SUBSPACE_YCBCR);
  if (!has_leaf(layer, WEED_LEAF_YUV_SAMPLING)) set_int(layer, WEED_LEAF_YUV_SAMPLING, WEED_YUV_SAMPLING_DEFAULT);
  return 1;
}

// K4 on a layer: the RGB24 / BGR24 / RGBA32 / BGRA32 / ARGB32 cases of src/colourspace.c:12559-12935 plus conv_done (:13860-13893)
lives_gpu_boolean rgb_layer_to_yuv(weed_plant_t *layer, const Layer &l_in, int outpl, int oclamping, int osubspace, int tgt_gamma, int flags) {
  // gamma on the way (:12311-12332): an RGB layer of known gamma that goes to YUV ends up SRGB (BT709 for a BT.709 target subspace) unless the caller names a
  // target.  The UYVY / YUYV entry points take the 16-bit LUT inline (can_inline_gamma :12136-12142, rgb2uyvy_with_gamma); for every other YUV palette the
  // reference converts the layer's gamma first (gamma_convert_layer, :12326-12329) and then the palette
  Layer l = l_in;
  int new_gamma = WEED_GAMMA_UNKNOWN;
  const bool inline_gamma = (outpl == WEED_PALETTE_UYVY || outpl == WEED_PALETTE_YUYV);
  const uint16_t *lut16 = nullptr;
  bool gamma_change = false;                      // the conversion needs a gamma change on the way: not recorded as LZ_SINK
  if (g_prefs.apply_gamma && l.gamma != WEED_GAMMA_UNKNOWN) {
    new_gamma = tgt_gamma != WEED_GAMMA_UNKNOWN ? tgt_gamma : osubspace == WEED_YUV_SUBSPACE_BT709 ? WEED_GAMMA_BT709 : WEED_GAMMA_SRGB;
    gamma_change = new_gamma != l.gamma;
    if (!inline_gamma) {
      if (new_gamma != l.gamma && !lives_gpu_gamma_convert_layer(new_gamma, layer)) return decline(layer);
      if (!read_layer(layer, &l)) return 0;
      new_gamma = l.gamma;
    } else if (new_gamma != l.gamma) {
      lut16 = device_lut16(l.gamma, new_gamma);          // nullptr when create_gamma_lut makes none for the pair: the plain entry point runs, as in the reference
    }
  }
  if (outpl == WEED_PALETTE_YUV411) return rgb_layer_to_yuv411(layer, l, oclamping, flags);
  const int fmt = k4_fmt(outpl);
  if (fmt < 0) return decline(layer);
  const int order = pal_order(l.pal);
  if (order == 2 && fmt >= 4) return decline(layer);                        // reference-broken (:6353)
  const int in_alpha = pal_has_alpha(l.pal) ? 1 : 0, out_alpha = pal_has_alpha(outpl) ? 1 : 0;
  int width = l.width, height = l.height;
  if (fmt >= 2 && (width & 1)) return decline(layer);
  if (fmt == 4) { width = (width >> 1) << 1; height = (height >> 1) << 1; }       // create_empty_pixel_data :11601-11603
  if (width < 2 || height < 1) return decline(layer);
  // subspace argument as the dispatcher passes it: some cases hand WEED_YUV_SAMPLING_DEFAULT (= 0 -> YCbCr) to the subspace slot
  const bool use_osub = (fmt == 4 && l.pal != WEED_PALETTE_RGB24) || (fmt == 5 && l.pal == WEED_PALETTE_RGB24);
  const int which = (oclamping == WEED_YUV_CLAMPING_UNCLAMPED ? 1 : 0) | ((fmt >= 4 && use_osub && osubspace == WEED_YUV_SUBSPACE_BT709) ? 2 : 0);
  const int lwidth = (fmt == 2 || fmt == 3) ? width >> 1 : width;                   // UYVY / YUYV layers count macropixels
  NewPlanes np;
  // RGBA32 / BGRA32 on a pinned layer to the sink's palette with no gamma change on the way: recorded as the program's last stage, LZ_SINK, not launched (deferred
  // execution, above).  A needed gamma change keeps the eager path below.  For UYVY / YUYV that is a matter of arithmetic (they take the 16-bit LUT inline there).
  // For the planar sinks it is only a limit of this stage: the lives_gpu_gamma_convert_layer above may itself have been recorded (LZ_LUT) and is materialised by the
  // eager conversion; LZ_LUT followed by LZ_SINK would be the same bytes (8-bit LUT, then K4) and could be recorded -- gamma_change, taken before that call, rules it out.
  const bool sink_pal = outpl == WEED_PALETTE_YUV420P || outpl == WEED_PALETTE_YVU420P || outpl == WEED_PALETTE_UYVY || outpl == WEED_PALETTE_YUYV;
  if (sink_pal && !gamma_change && lazy_pal(l.pal)) {
    if (Lazy *z = lazy_detach(l, LZ_SINK)) {
      if (!alloc_planes(outpl, lwidth, height, 0, &np)) { lazy_reattach(l.pd[0], z); return 0; }
      z->sink = true; z->stage = LZ_SINK; z->sfmt = fmt; z->swhich = which; z->sorder = order; z->snp = np.n; z->sww = width; z->shh = height;
      for (int p = 0; p < np.n; p++) { z->sors[p] = np.rs[p]; z->sbytes[p] = np.sz[p]; z->sph[p] = np.pd[p]; }
      g_lz_recorded++; g_lz_sink_recorded++;
      for (int p = 0; p < np.n; p++) {                                               // one entry per plane, all pointing at the program
        Dev e;
        e.lazy = z; e.bytes = np.sz[p]; e.stream = kIdle;
        const Dev old = res_swap(np.pd[p], e);
        if (old.d || old.lazy) pool_give(old);
      }
      free_host_planes(l);                // free_planes without the table (the entry has moved)
      swap_chroma_planes(outpl, &np);
      commit_planes(layer, outpl, lwidth, height, np);
      if (flags != l.flags) set_int(layer, kLeafHostFlags, flags);
      set_int(layer, WEED_LEAF_YUV_CLAMPING, oclamping);
      if (inline_gamma && new_gamma != WEED_GAMMA_UNKNOWN) set_int(layer, WEED_LEAF_GAMMA_TYPE, new_gamma);                                   // (== l.gamma here)
      set_int(layer, WEED_LEAF_YUV_SUBSPACE, l.gamma == WEED_GAMMA_BT709 ? WEED_YUV_SUBSPACE_BT709 : WEED_YUV_SUBSPACE_YCBCR);
      if (fmt >= 4 || !has_leaf(layer, WEED_LEAF_YUV_SAMPLING)) set_int(layer, WEED_LEAF_YUV_SAMPLING, WEED_YUV_SAMPLING_DEFAULT);
      return 1;
    }
  }
  if (!alloc_planes(outpl, lwidth, height, 0, &np)) return 0;
  Work w;
  const uint8_t *d_in = w.in(l.pd[0], (size_t)l.rs[0] * l.height, 0);
  uint8_t *ddst[4] = {nullptr, nullptr, nullptr, nullptr};
  int ors[4] = {0, 0, 0, 0};
  for (int p = 0; p < np.n; p++) { ddst[p] = w.out(np.pd[p], np.sz[p], 3 + p, true); ors[p] = np.rs[p]; }   // calloc'd padding stays as the host made it
  const bool ok = w.ok &&
                  (lut16 ? lgpu_rgb_to_yuv_lut16(d_in, l.rs[0], width, height, order, in_alpha, ddst[0], ors[0], fmt, which & 1, lut16, S())
                         : lgpu_rgb_to_yuv(d_in, l.rs[0], width, height, order, in_alpha, ddst, ors, fmt, out_alpha, which, S())) == LGPU_OK &&
                  w.finish();
  if (!ok) { drop_new_planes(np); return 0; }
  free_planes(l);
  swap_chroma_planes(outpl, &np);
  commit_planes(layer, outpl, lwidth, height, np);
  if (flags != l.flags) set_int(layer, kLeafHostFlags, flags);
  set_int(layer, WEED_LEAF_YUV_CLAMPING, oclamping);
  int final_gamma = l.gamma;
  if (inline_gamma && new_gamma != WEED_GAMMA_UNKNOWN) { set_int(layer, WEED_LEAF_GAMMA_TYPE, new_gamma); final_gamma = new_gamma; }      // :13873-13876
  set_int(layer, WEED_LEAF_YUV_SUBSPACE, final_gamma == WEED_GAMMA_BT709 ? WEED_YUV_SUBSPACE_BT709 : WEED_YUV_SUBSPACE_YCBCR);              // :13884-13888
  if (fmt >= 4 || !has_leaf(layer, WEED_LEAF_YUV_SAMPLING)) set_int(layer, WEED_LEAF_YUV_SAMPLING, WEED_YUV_SAMPLING_DEFAULT);
  return 1;
}

}  // namespace

extern "C" {

int lives_gpu_bind_weed(const lives_gpu_weed_api *api) {
  if (!api || !api->leaf_get || !api->leaf_set || !api->leaf_num_elements || !api->leaf_delete) return LGPU_E_BADARG;
  g_api = *api;
  return LGPU_OK;
}

int lives_gpu_bind_leaf_get_flags(weed_leaf_get_flags_f leaf_get_flags) {
  g_leaf_get_flags = leaf_get_flags;
  return LGPU_OK;
}

int lives_gpu_set_prefs(const lives_gpu_prefs *prefs) {
  if (!prefs) return LGPU_E_BADARG;
  g_prefs = *prefs;
  return LGPU_OK;
}


int *lives_gpu_calc_rowstrides(int width, int pal, lives_gpu_layer_t *layer, int *nplanes) {
  if (pal == WEED_PALETTE_NONE) { if (!layer || !bound()) return nullptr; pal = get_int(layer, WEED_LEAF_CURRENT_PALETTE, 0); }
  if (!width) { if (!layer || !bound()) return nullptr; width = get_int(layer, WEED_LEAF_WIDTH, 0); }
  int rs[4];
  const int n = lgpu_calc_rowstrides(width, pal, take_alignment(0), rs);
  if (nplanes) *nplanes = n;
  if (!n) return nullptr;
  apply_const_rowstrides(layer, n, rs);
  int *out = (int *)calloc((size_t)n, sizeof(int));      // caller frees with lives_free, like the reference
  for (int i = 0; i < n; i++) out[i] = rs[i];
  return out;
}

// YUV -> YUV repack of a layer (:12937-13750, the non-RGB half of the dispatcher) through lgpu_yuv_repack; 0 = not taken, the
// caller's CPU body runs (pairs / layouts listed in include/lives_gpu.h)
static lives_gpu_boolean yuv_layer_repack(weed_plant_t *layer, const Layer &l, int outpl, int iclamping, int flags) {
  const int inpl = l.pal;
  const bool inpk = (inpl == WEED_PALETTE_UYVY || inpl == WEED_PALETTE_YUYV), outpk = (outpl == WEED_PALETTE_UYVY || outpl == WEED_PALETTE_YUYV);
  const bool in411 = inpl == WEED_PALETTE_YUV411, out411 = outpl == WEED_PALETTE_YUV411;
  const int width = inpk ? l.width * 2 : in411 ? l.width * 4 : l.width, height = l.height;              // pixels
  if (width < 1 || height < 1) return decline(layer);
  const int unclamped = iclamping == WEED_YUV_CLAMPING_UNCLAMPED ? 1 : 0;
  const uint8_t *dsrc[4] = {nullptr, nullptr, nullptr, nullptr};
  uint8_t *ddst[4] = {nullptr, nullptr, nullptr, nullptr};
  int irs[4] = {0, 0, 0, 0}, ors[4] = {0, 0, 0, 0};
  Work w;
  if (inpk && outpk) {
    // convert_swab_frame (:13139): in place, the layer keeps its pixel data
    uint8_t *dd[4] = {w.inout(l.pd[0], (size_t)l.rs[0] * height, 0), nullptr, nullptr, nullptr};
    dsrc[0] = dd[0]; irs[0] = l.rs[0];
    if (!w.ok) return 0;
    const int rc = lgpu_yuv_repack(inpl, outpl, dsrc, irs, dd, irs, width, height, unclamped, 0, S());
    if (rc == LGPU_E_UNSUPPORTED) return decline(layer);
    if (rc != LGPU_OK || !w.finish()) return 0;
    set_int(layer, WEED_LEAF_CURRENT_PALETTE, outpl);
    return 1;
  }
  for (int p = 0; p < l.nplanes; p++) { dsrc[p] = w.in(l.pd[p], (size_t)l.rs[p] * plane_h(l, p), p == 3 ? 7 : p); irs[p] = l.rs[p]; }
  if (!w.ok) return 0;
  if (inpl == WEED_PALETTE_YVU420P) { const uint8_t *t = dsrc[1]; dsrc[1] = dsrc[2]; dsrc[2] = t; const int r = irs[1]; irs[1] = irs[2]; irs[2] = r; }
  // K5c, the 4:1:1 pairs (:13024-13029 ..., :13793-13846): the new layer gets its ordinary (aligned, zeroed) planes and the reference functions then walk
  // them as compact streams; lgpu_yuv_repack does the same
  if ((in411 || out411) && (width & 3)) return decline(layer);
  if (in411 && (outpl == WEED_PALETTE_YUV420P || outpl == WEED_PALETTE_YVU420P) && (height & 1)) return decline(layer);
  const int lwidth = outpk ? width >> 1 : out411 ? width >> 2 : width;
  NewPlanes np;
  if (!alloc_planes(outpl, lwidth, height, 0, &np)) return 0;
  for (int p = 0; p < np.n; p++) { ddst[p] = w.out(np.pd[p], np.sz[p], 3 + p, true); ors[p] = np.rs[p]; }
  const int rc = w.ok ? lgpu_yuv_repack(inpl, outpl, dsrc, irs, ddst, ors, width, height, unclamped, l.sampling, S()) : LGPU_E_NOMEM;   // isampling: read by K5d only
  if (rc == LGPU_E_UNSUPPORTED) { drop_new_planes(np); return decline(layer); }
  if (rc != LGPU_OK || !w.finish()) { drop_new_planes(np); return 0; }
  free_planes(l);
  swap_chroma_planes(outpl, &np);
  commit_planes(layer, outpl, lwidth, height, np);
  if (flags != l.flags) set_int(layer, kLeafHostFlags, flags);
  if ((outpl == WEED_PALETTE_YUV420P || outpl == WEED_PALETTE_YVU420P) && !in411) set_int(layer, WEED_LEAF_YUV_SAMPLING, WEED_YUV_SAMPLING_DEFAULT);   // :13022
  return 1;
}

// black of a palette as the reference paints it (blank_pixel / blank_row, src/colourspace.c:11123-11210) into a HOST plane set
static void host_black_fill(int pal, int width, int height, int clamping, const NewPlanes &np) {
  const uint8_t yb = clamping == WEED_YUV_CLAMPING_UNCLAMPED ? 0 : 16;
  if (pal_is_planar_yuv(pal)) {
    for (int p = 0; p < np.n; p++) memset(np.pd[p], p == 0 ? yb : p == 3 ? 255 : 128, np.sz[p]);
  } else if (pal_has_alpha(pal)) {
    const int a = pal_alpha_first(pal) ? 0 : 3;
    for (int y = 0; y < height; y++) for (int x = 0; x < width; x++) np.pd[0][(size_t)y * np.rs[0] + x * 4 + a] = 255;
  }
}

lives_gpu_boolean lives_gpu_create_empty_pixel_data(lives_gpu_layer_t *layer, lives_gpu_boolean black_fill, lives_gpu_boolean may_contig) {
  (void)may_contig;
  if (!layer || !bound()) return 0;
  const int pal = get_int(layer, WEED_LEAF_CURRENT_PALETTE, 0);
  int width = get_int(layer, WEED_LEAF_WIDTH, 0), height = get_int(layer, WEED_LEAF_HEIGHT, 0);
  if (width <= 0 || height <= 0 || !pal_psize(pal)) return 0;
  if (pal == WEED_PALETTE_YUV420P || pal == WEED_PALETTE_YVU420P) { width = (width >> 1) << 1; height = (height >> 1) << 1; }   // :11601-11603
  Layer old;
  const bool had = read_layer(layer, &old);
  NewPlanes np;
  if (!alloc_planes(pal, width, height, 0, &np, layer, true)) return 0;
  // opaque black: RGB 0,0,0 (alpha 255); YUV 16 (clamped) or 0, 128, 128 (src/colourspace.c:11448-11460)
  if (black_fill) host_black_fill(pal, width, height, get_int(layer, WEED_LEAF_YUV_CLAMPING, WEED_YUV_CLAMPING_UNCLAMPED), np);
  if (had) free_planes(old);
  commit_planes(layer, pal, width, height, np);
  return 1;
}

static lives_gpu_boolean convert_layer_palette_full(lives_gpu_layer_t *layer, int outpl, int oclamping, int osampling, int osubspace, int tgt_gamma) {
  Layer l;
  if (!ready() || !read_layer(layer, &l)) return 0;
  const int inpl = l.pal;
  // The reference's own first steps (range switch :12241-12262, un-premultiply :12290-12306) are done first here too.  If the
  // conversion proper is then declined, the layer is in the state the reference has at that point and its CPU body continues from
  // there (both steps are no-ops the second time: the leaves they test have been updated).
  if (pal_is_yuv(inpl) && pal_is_yuv(outpl) && ((l.clamping >= 0 && l.clamping != oclamping) || l.subspace != osubspace)) {      // :12241 (iclamping = oclamping without the leaf, :12216-12218)
    // YUV -> YUV with a different range: same subspace = in-place table switch (:12242-12247); a subspace change goes through RGB(A) (:12248-12262) -- the
    // frame is taken to RGB24 / RGBA32 with its own tables and converted from there with the target's range and subspace, as the reference does it
    if (l.subspace != osubspace) {
      if (!lives_gpu_convert_layer_palette(layer, pal_has_alpha(inpl) ? WEED_PALETTE_RGBA32 : WEED_PALETTE_RGB24, 0)) return 0;
      return convert_layer_palette_full(layer, outpl, oclamping, osampling, osubspace, tgt_gamma);
    }
    if (!switch_layer_clamping(layer, l, oclamping)) return 0;
    if (!read_layer(layer, &l)) return 0;
  }
  if (inpl == outpl) {                                                     // :12265
    // Nothing left to do, exactly as in the reference: its 4:2:0 JPEG <-> MPEG chroma-siting pass (switch_yuv_sampling, :10876-10925) is called
    // from inside `if (isampling == osampling && ...)` under the condition `isampling != osampling` (:12268-12274), i.e. never (quirk SS1): a request
    // that differs in sampling only returns TRUE with the pixels and the YUV_sampling leaf as they were.
    return 1;
  }
  // premultiplied-alpha bookkeeping (:12290-12306), for every in / out palette pair
  int flags = l.flags;
  if (g_prefs.alpha_post) {
    if ((flags & LIVES_LAYER_ALPHA_PREMULT) && pal_has_alpha(inpl) && !pal_has_alpha(outpl)) {
      lives_gpu_alpha_premult(layer, LIVES_DIRECTION_REVERSE);
      if (!read_layer(layer, &l)) return 0;
      flags = l.flags;
    }
  } else if (!pal_has_alpha(inpl) && pal_has_alpha(outpl)) flags |= LIVES_LAYER_ALPHA_PREMULT;
  if (pal_has_alpha(inpl) && !pal_has_alpha(outpl)) flags &= ~LIVES_LAYER_ALPHA_PREMULT;

  if (!pal_is_rgb(outpl)) {
    if (pal_is_rgb(inpl)) return rgb_layer_to_yuv(layer, l, outpl, oclamping, osubspace, tgt_gamma, flags);
    return yuv_layer_repack(layer, l, outpl, l.clamping >= 0 ? l.clamping : oclamping, flags);   // YUV -> YUV repacks (K5b)
  }
  const int iclamping = l.clamping >= 0 ? l.clamping : oclamping;        // :12216-12218

  // gamma decision (:12311-12332): only an explicit target changes the transfer function here
  int new_gamma = l.gamma;
  uint8_t lut[256];
  const uint8_t *lutp = nullptr;
  if (g_prefs.apply_gamma && l.gamma != WEED_GAMMA_UNKNOWN && tgt_gamma != WEED_GAMMA_UNKNOWN && tgt_gamma != l.gamma) {
    new_gamma = tgt_gamma;
    if (lgpu_gamma_lut8(1.0, l.gamma, new_gamma, g_prefs.screen_gamma, lut)) lutp = lut;
  }
  const bool in_planar_sub = (inpl == WEED_PALETTE_YUV420P || inpl == WEED_PALETTE_YVU420P || inpl == WEED_PALETTE_YUV422P);
  if (!pal_is_rgb(inpl) && !in_planar_sub && k3_fmt(inpl) < 0 && inpl != WEED_PALETTE_YUV411) return decline(layer);
  if (lutp && !pal_is_rgb(inpl) && !in_planar_sub) return decline(layer);   // no inline gamma on the K3 / 4:1:1 paths

  if (!lutp && lazy_pal(inpl) && lazy_pal(outpl)) {
    // RGBA32 <-> BGRA32 on a pinned layer: recorded, not launched (deferred execution, above)
    if (Lazy *z = lazy_detach(l, LZ_SWAP)) {
      const int prev = z->stage;
      z->swap = true; z->stage = LZ_SWAP;
      if (!lazy_commit(layer, l, z, outpl, l.width, l.height, 0)) { z->swap = false; z->stage = prev; lazy_reattach(l.pd[0], z); return 0; }
      if (new_gamma != l.gamma) set_int(layer, WEED_LEAF_GAMMA_TYPE, new_gamma);
      if (flags != l.flags) set_int(layer, kLeafHostFlags, flags);
      delete_yuv_leaves(layer);
      return 1;
    }
  }
  if (!lutp && (in_planar_sub || inpl == WEED_PALETTE_UYVY || inpl == WEED_PALETTE_YUYV) && lazy_pal(outpl) &&
      lazy_record_yuv(layer, l, outpl, (iclamping == WEED_YUV_CLAMPING_UNCLAMPED ? 1 : 0) | (l.subspace == WEED_YUV_SUBSPACE_BT709 ? 2 : 0), new_gamma, flags))
    return 1;                                   // a decoder frame on a pinned layer: recorded, not launched (deferred execution, above)
  NewPlanes np;
  const int owidth = (inpl == WEED_PALETTE_UYVY || inpl == WEED_PALETTE_YUYV) ? l.width * 2 : inpl == WEED_PALETTE_YUV411 ? l.width * 4 : l.width;   // macropixels -> pixels (:13010, :13759)
  if (!alloc_planes(outpl, owidth, l.height, 0, &np)) return 0;
  const size_t obytes = (size_t)np.rs[0] * l.height;
  Work w;
  bool ok = true;
  if (pal_is_rgb(inpl)) {
    int af = 0;
    const int op = rgb_swizzle_op(inpl, outpl, &af);
    const uint8_t *d_in = w.in(l.pd[0], (size_t)l.rs[0] * l.height, 0);
    uint8_t *d_out = w.out(np.pd[0], obytes, 3, true);
    ok = w.ok && lgpu_swizzle(op, af, d_in, l.rs[0], d_out, np.rs[0], l.width, l.height, lutp, S()) == LGPU_OK;
  } else if (in_planar_sub) {
    const int iu = (inpl == WEED_PALETTE_YVU420P) ? 2 : 1, iv = (inpl == WEED_PALETTE_YVU420P) ? 1 : 2;   // swap_chroma_planes (:12353)
    const int ch = plane_h(l, 1);
    const size_t yb = (size_t)l.rs[0] * l.height, ub = (size_t)l.rs[iu] * ch, vb = (size_t)l.rs[iv] * ch;
    const uint8_t *dy = w.in(l.pd[0], yb, 0), *du = w.in(l.pd[iu], ub, 1), *dv = w.in(l.pd[iv], vb, 2);
    uint8_t *d_out = w.out(np.pd[0], obytes, 3, np.rs[0] != l.width * pal_psize(outpl));     // the kernel writes every byte of every pixel: only row padding needs the zeros
    const int strides[3] = {l.rs[0], l.rs[iu], l.rs[iv]};
    const int which = (iclamping == WEED_YUV_CLAMPING_UNCLAMPED ? 1 : 0) | (l.subspace == WEED_YUV_SUBSPACE_BT709 ? 2 : 0);
    const int order = pal_order(outpl);
    ok = w.ok;
    if (ok && lutp) {
      // with a target gamma the reference fuses the 16-bit indexed LUT of create_gamma_lut into the conversion (:3274-3283)
      const uint16_t *d16 = device_lut16(l.gamma, new_gamma);
      ok = d16 && lgpu_yuv420p_to_rgb_lut16(dy, du, dv, strides, (long)ub, (long)vb, d_out, np.rs[0], l.width, l.height, pal_psize(outpl), order,
                                            inpl == WEED_PALETTE_YUV422P, which, g_prefs.pb_quality, d16, 0, S()) == LGPU_OK;
    } else if (ok)
      ok = lgpu_yuv420p_to_rgb(dy, du, dv, strides, (long)ub, (long)vb, d_out, np.rs[0], l.width, l.height, pal_psize(outpl), order,
                               inpl == WEED_PALETTE_YUV422P, which, g_prefs.pb_quality, nullptr, 0, S()) == LGPU_OK;
  } else if (k3_fmt(inpl) >= 0) {
    // K3: packed / planar 4:4:4, UYVY, YUYV -> RGB family (src/colourspace.c:12937-13860 cases); no inline gamma on these paths
    const int fmt = k3_fmt(inpl), in_alpha = (inpl == WEED_PALETTE_YUVA8888 || inpl == WEED_PALETTE_YUVA4444P);
    const int pxw = (fmt >= 2) ? l.width * 2 : l.width;                     // UYVY / YUYV layers count macropixels
    const int order = pal_order(outpl);
    const int which = (iclamping == WEED_YUV_CLAMPING_UNCLAMPED ? 1 : 0) | ((fmt == 0 && l.subspace == WEED_YUV_SUBSPACE_BT709) ? 2 : 0);
    if (fmt >= 2 && np.rs[0] < pxw * pal_psize(outpl)) { drop_new_planes(np); return decline(layer); }
    const uint8_t *dsrc[4] = {nullptr, nullptr, nullptr, nullptr};
    int irs[4] = {0, 0, 0, 0};
    for (int p = 0; p < l.nplanes; p++) { dsrc[p] = w.in(l.pd[p], (size_t)l.rs[p] * l.height, p == 0 ? 0 : p + 3); irs[p] = l.rs[p]; }
    uint8_t *d_out = w.out(np.pd[0], obytes, 3, true);
    ok = w.ok && lgpu_yuv_to_rgb(dsrc, irs, pxw, l.height, fmt, in_alpha, d_out, np.rs[0], order, pal_has_alpha(outpl) ? 1 : 0, which, S()) == LGPU_OK;
  } else {
    // K3b, YUV411 (:13755-13795): the reference walks the source as compact rows of `width` macropixels and leaves some alpha bytes of the
    // new (zeroed, create_empty_pixel_data) frame unwritten -- the device frame starts zeroed too
    const size_t ibytes = (size_t)l.width * 6 * l.height;
    const int order = pal_order(outpl);
    if ((size_t)l.rs[0] * l.height < ibytes) { drop_new_planes(np); return decline(layer); }
    const uint8_t *d_in = w.in(l.pd[0], ibytes, 0);
    uint8_t *d_out = w.out(np.pd[0], obytes, 3, true);
    ok = w.ok && lgpu_yuv411_to_rgb(d_in, l.width, l.height, d_out, np.rs[0], order, pal_has_alpha(outpl) ? 1 : 0,
                                   iclamping == WEED_YUV_CLAMPING_UNCLAMPED, S()) == LGPU_OK;
  }
  ok = ok && w.finish();
  if (!ok) { drop_new_planes(np); return 0; }                                // memfail: layer untouched
  free_planes(l);
  commit_planes(layer, outpl, owidth, l.height, np);
  if (new_gamma != l.gamma) set_int(layer, WEED_LEAF_GAMMA_TYPE, new_gamma);
  if (flags != l.flags) set_int(layer, kLeafHostFlags, flags);
  delete_yuv_leaves(layer);
  return 1;
}
lives_gpu_boolean lives_gpu_convert_layer_palette_full(lives_gpu_layer_t *layer, int outpl, int oclamping, int osampling,
                                                       int osubspace, int tgt_gamma) {
  return pinned(layer, [&] { return convert_layer_palette_full(layer, outpl, oclamping, osampling, osubspace, tgt_gamma); });
}

lives_gpu_boolean lives_gpu_convert_layer_palette(lives_gpu_layer_t *layer, int outpl, int op_clamping) {
  return lives_gpu_convert_layer_palette_full(layer, outpl, op_clamping, WEED_YUV_SAMPLING_DEFAULT, WEED_YUV_SUBSPACE_YUV, WEED_GAMMA_UNKNOWN);   // :13931
}

// src/colourspace.c:13935-13938
lives_gpu_boolean lives_gpu_convert_layer_palette_with_sampling(lives_gpu_layer_t *layer, int outpl, int out_sampling) {
  return lives_gpu_convert_layer_palette_full(layer, outpl, WEED_YUV_CLAMPING_UNCLAMPED, out_sampling, WEED_YUV_SUBSPACE_YUV, WEED_GAMMA_UNKNOWN);
}

static lives_gpu_boolean gamma_convert_sub_layer(int gamma_type, double fileg, lives_gpu_layer_t *layer, int x, int y, int width, int height) {
  if (!g_prefs.apply_gamma) return 1;
  Layer l;
  if (!ready() || !read_layer(layer, &l)) return 0;
  if (!pal_is_rgb(l.pal)) return decline(layer);
  if (gamma_type == l.gamma && fileg == 1.0) return 1;
  uint8_t lut[256];
  {
    // the calling thread's last table is kept, as the reference keeps its last one (:664-670): 255 powf pairs per call otherwise
    thread_local struct { double fg, sg; int from, to, made; uint8_t t[256]; } memo = {0., 0., 0, 0, -1, {0}};
    const double fg = gamma_type == LIVES_GAMMA_VARIANT ? fileg : 1.0;
    if (!(memo.made >= 0 && memo.fg == fg && memo.sg == g_prefs.screen_gamma && memo.from == l.gamma && memo.to == gamma_type)) {
      memo.made = lgpu_gamma_lut8(fg, l.gamma, gamma_type, g_prefs.screen_gamma, memo.t);
      memo.fg = fg; memo.sg = g_prefs.screen_gamma; memo.from = l.gamma; memo.to = gamma_type;
    }
    if (!memo.made) return 1;
    memcpy(lut, memo.t, 256);
  }
  if (x < 0 || y < 0 || x + width > l.width || y + height > l.height) return 0;
  if (x == 0 && y == 0 && width == l.width && height == l.height && lazy_pal(l.pal) && plane_is_lazy(l.pd[0])) {
    // the whole frame of a plane that is still a pending program: the table becomes its last stage
    if (Lazy *z = lazy_detach(l, LZ_LUT)) {
      if (z->stage != LZ_NONE) {
        z->lut = true; memcpy(z->lut8, lut, 256); z->stage = LZ_LUT;
        lazy_attach(l.pd[0], z);
        if (gamma_type != LIVES_GAMMA_VARIANT) set_int(layer, WEED_LEAF_GAMMA_TYPE, gamma_type);
        return 1;
      }
      lazy_reattach(l.pd[0], z);          // the program had a table already and has run: a table pass alone is one kernel, in place, below
    }
  }
  Work w;
  uint8_t *d = w.inout(l.pd[0], (size_t)l.rs[0] * l.height, 0);
  const bool ok = w.ok && lgpu_gamma_apply(d, l.rs[0], x, y, width, height, pal_psize(l.pal), pal_alpha_first(l.pal), lut, S()) == LGPU_OK && w.finish();
  if (!ok) return 0;
  if (gamma_type != LIVES_GAMMA_VARIANT) set_int(layer, WEED_LEAF_GAMMA_TYPE, gamma_type);
  return 1;
}
lives_gpu_boolean lives_gpu_gamma_convert_sub_layer(int gamma_type, double fileg, lives_gpu_layer_t *layer, int x, int y, int width,
                                                    int height, lives_gpu_boolean may_thread) {
  (void)may_thread;
  return pinned(layer, [&] { return gamma_convert_sub_layer(gamma_type, fileg, layer, x, y, width, height); });
}

lives_gpu_boolean lives_gpu_gamma_convert_layer(int gamma_type, lives_gpu_layer_t *layer) {
  Layer l;
  if (!bound() || !read_layer(layer, &l)) return 0;
  return lives_gpu_gamma_convert_sub_layer(gamma_type, 1.0, layer, 0, 0, l.width, l.height, 1);   // :14146-14155
}

// gamma_convert_layer_variant (src/colourspace.c:14157-14168): the layer is tagged LINEAR, then taken to tgt_gamma through
// gamma_convert_sub_layer(tgt_gamma, file_gamma, ...): as there, file_gamma enters the table only when tgt_gamma is WEED_GAMMA_VARIANT
// (:14099-14102) -- kept
lives_gpu_boolean lives_gpu_gamma_convert_layer_variant(double file_gamma, int tgt_gamma, lives_gpu_layer_t *layer) {
  Layer l;
  if (!bound() || !read_layer(layer, &l)) return 0;
  set_int(layer, WEED_LEAF_GAMMA_TYPE, WEED_GAMMA_LINEAR);
  return lives_gpu_gamma_convert_sub_layer(tgt_gamma, file_gamma, layer, 0, 0, l.width, l.height, 1);
}

void lives_gpu_alpha_premult(lives_gpu_layer_t *layer, int direction) {
  PinScope pin(layer);
  Layer l;
  if (!ready() || !read_layer(layer, &l) || !pal_has_alpha(l.pal)) return;
  Work w;
  bool ok = true;
  if (l.pal == WEED_PALETTE_YUVA8888 || l.pal == WEED_PALETTE_YUVA4444P) {
    // :11982, :12005-12047, :12063-12096: clamped layers go through the alcy / alcuv / unalcy / unalcuv tables, unclamped ones through al / unal
    const int clamped = (l.clamping < 0 || l.clamping == WEED_YUV_CLAMPING_CLAMPED) ? 1 : 0;      // weed_layer_get_yuv_clamping(): CLAMPED (0) when the leaf is missing
    uint8_t *dp[4] = {nullptr, nullptr, nullptr, nullptr};
    int rs[4] = {0, 0, 0, 0};
    for (int p = 0; p < l.nplanes; p++) {
      const size_t nb = (size_t)l.rs[p] * l.height;
      dp[p] = (p == 3) ? const_cast<uint8_t *>(w.in(l.pd[p], nb, 7)) : w.inout(l.pd[p], nb, p);           // the alpha plane is only read
      rs[p] = l.rs[p];
    }
    ok = w.ok && lgpu_alpha_premult_yuva(dp, rs, l.width, l.height, l.pal, clamped, direction == LIVES_DIRECTION_REVERSE, S()) == LGPU_OK;
  } else {
    uint8_t *d = w.inout(l.pd[0], (size_t)l.rs[0] * l.height, 0);
    ok = w.ok && lgpu_alpha_premult(d, l.rs[0], l.width, l.height, pal_alpha_first(l.pal), direction == LIVES_DIRECTION_REVERSE, S()) == LGPU_OK;
  }
  if (!ok || !w.finish()) return;
  int flags = l.flags;
  if (direction == LIVES_DIRECTION_FORWARD) flags |= LIVES_LAYER_ALPHA_PREMULT; else flags &= ~LIVES_LAYER_ALPHA_PREMULT;   // :12098-12102
  set_int(layer, kLeafHostFlags, flags);
}

// resize every plane of `l` into freshly allocated planes of (width x height); lut8: the fused post-pass of :14718-14720 (RGB only)
static bool resize_into(const Layer &l, int width, int height, int interp, int alignment, const uint8_t *lut8, NewPlanes *np) {
  if (!alloc_planes(l.pal, width, height, alignment, np)) return false;
  Work w;
  Layer nl = l;
  nl.width = width; nl.height = height;
  bool ok = true;
  for (int p = 0; p < np->n && ok; p++) {
    const int ps = pal_is_planar_yuv(l.pal) ? 1 : pal_psize(l.pal);
    const int sw = plane_w(l, p), sh = plane_h(l, p), dw = plane_w(nl, p), dh = plane_h(nl, p);
    const uint8_t *d_in = w.in(l.pd[p], (size_t)l.rs[p] * sh, p == 3 ? 7 : p);          // scratch slots (ordinary layers): planes in 0, 1, 2, 7; planes out 3 .. 6
    uint8_t *d_out = w.out(np->pd[p], (size_t)np->rs[p] * dh, 3 + p, np->rs[p] != dw * ps);          // zeros for the row padding only
    ok = w.ok && lgpu_resize(d_in, l.rs[p], sw, sh, d_out, np->rs[p], dw, dh, ps, interp, lut8, S()) == LGPU_OK;
  }
  ok = ok && w.finish();
  if (!ok) drop_new_planes(*np);
  return ok;
}

// What resize_layer_full decides before it scales (shared with letterbox_layer, which scales straight into its canvas): the layer converted to a resizable
// palette if need be, the even source size, the adjusted target size, the fused gamma table.  Returns 1 = scale, 0 = failed / declined (*rc says which
// value the seam call returns), 2 = nothing to do.
namespace { struct ResizePlan { Layer l, src; int width, height, new_gamma; bool use_lut; uint8_t lut[256]; }; }
static int plan_resize(weed_plant_t *layer, int width, int height, int opal_hint, int osubs_hint, int tgt_gamma, ResizePlan *rp, int *rc) {
  Layer &l = rp->l;
  *rc = 0;
  if (!ready() || !read_layer(layer, &l)) return 0;
  // opal_hint / oclamp_hint "may be ignored ... layer palette should be checked on return" (:14746-14751): a frame whose palette this path
  // resizes keeps it (the caller's following convert_layer_palette does the rest); a packed-YUV frame is first taken to the hinted
  // palette when that one is resizable and the conversion is served here
  if (!(pal_is_rgb(l.pal) || pal_is_planar_yuv(l.pal))) {
    if (opal_hint == WEED_PALETTE_NONE || opal_hint == l.pal || !(pal_is_rgb(opal_hint) || pal_is_planar_yuv(opal_hint))) { *rc = decline(layer); return 0; }
    const int cl = l.clamping >= 0 ? l.clamping : WEED_YUV_CLAMPING_CLAMPED;
    if (!lives_gpu_convert_layer_palette_full(layer, opal_hint, cl, WEED_YUV_SAMPLING_DEFAULT, l.subspace, WEED_GAMMA_UNKNOWN)) return 0;
    if (!read_layer(layer, &l)) return 0;
  }
  int iwidth = (l.width >> 1) << 1, iheight = (l.height >> 1) << 1;      // :14854-14863
  if (width < 4) width = 4;
  if (height < 4) height = 4;
  if (iwidth != width || iheight != height) height = (height >> 1) << 1;
  if (iwidth == width && iheight == height) { *rc = 1; return 2; }
  if (pal_is_planar_yuv(l.pal)) width = (width >> 1) << 1;
  // target gamma (:14890-14899, :15119-15127): applied as a LUT8 after the scaler when the output is RGB and the layer's gamma is known
  const int opal = (opal_hint == WEED_PALETTE_NONE || opal_hint == WEED_PALETTE_ANY) ? l.pal : opal_hint;
  if (tgt_gamma == WEED_GAMMA_UNKNOWN && !pal_is_rgb(opal) && osubs_hint == WEED_YUV_SUBSPACE_BT709) tgt_gamma = WEED_GAMMA_BT709;
  if (tgt_gamma == WEED_GAMMA_UNKNOWN && pal_is_rgb(l.pal) && !pal_is_rgb(opal)) tgt_gamma = WEED_GAMMA_SRGB;       // get_tgt_gamma :14733
  if (tgt_gamma == WEED_GAMMA_UNKNOWN) tgt_gamma = l.gamma;
  rp->use_lut = false;
  rp->new_gamma = l.gamma;
  if (tgt_gamma != WEED_GAMMA_UNKNOWN && pal_is_rgb(opal) && pal_is_rgb(l.pal)) {
    if (l.gamma != WEED_GAMMA_UNKNOWN && l.gamma != tgt_gamma && lgpu_gamma_lut8(1.0, l.gamma, tgt_gamma, g_prefs.screen_gamma, rp->lut)) rp->use_lut = true;
    rp->new_gamma = tgt_gamma;
  }
  rp->src = l;
  rp->src.width = iwidth; rp->src.height = iheight;
  rp->width = width; rp->height = height;
  return 1;
}

// ---- resize backend ------------------------------------------------------------------------------------------------------------------
// resize_layer_full has two bodies in the reference: the swscale one (:14940-15259; un-vendored, version unpinned -> this library's own
// polyphase spec) and the gdk-pixbuf one (:15262-15322: layer_to_pixbuf, lives_pixbuf_scale_simple, pixbuf_to_layer).
// The second is pinned byte for byte (pixbuf.hip) and is the DEFAULT: a host that links the seam and calls resize_layer / letterbox_layer as the
// reference does gets arithmetic a reference binary pins.  The polyphase body is the opt-in of a host "built with USE_SWSCALE".
static std::atomic<int> g_resize_backend{LIVES_GPU_RESIZE_PIXBUF};
int lives_gpu_set_resize_backend(int backend) {
  if (backend != LIVES_GPU_RESIZE_POLYPHASE && backend != LIVES_GPU_RESIZE_PIXBUF) return -1;
  g_resize_backend.store(backend);
  return 0;
}
int lives_gpu_get_resize_backend(void) { return g_resize_backend.load(); }

static bool pal_is_pixbuf(int pal) {      // the cases of the switch at :15275-15290 (3 or 4 channels, alpha last)
  return pal == WEED_PALETTE_RGB24 || pal == WEED_PALETTE_BGR24 || pal == WEED_PALETTE_RGBA32 || pal == WEED_PALETTE_BGRA32 ||
         pal == WEED_PALETTE_YUV888 || pal == WEED_PALETTE_YUVA8888;
}

// ---- the palette resolution in front of the resize bodies, and the planner's capability queries (src/colourspace.h:400-407) ------------------------------
// The reference answers these from its CPU rules; exported under the reference's names by liblivesgpu_dropin.so, they describe the bodies of THIS library, so
// that a planner which swapped the bodies plans for what will run (callers: src/nodemodel.c:131, :143, :210, :2961).
// weed_palette_is_resizable (:2647-2654) for the body in force.  PIXBUF: the switch of a build without swscale (weed_palette_conv_resizable, :2619-2643), which is
// also the switch of the gdk-pixbuf body itself (:15275-15290).  POLYPHASE: what that body scales as it comes (packed RGB, planar YUV).
static bool pal_resizable(int pal) {
  if (g_resize_backend.load() == LIVES_GPU_RESIZE_PIXBUF) return pal_is_pixbuf(pal);
  return pal_is_rgb(pal) || pal_is_planar_yuv(pal);
}
static int masq_pal(int pal) {                                         // get_masq_pal (:14500-14513)
  if (g_resize_backend.load() != LIVES_GPU_RESIZE_PIXBUF) return WEED_PALETTE_NONE;      // the polyphase body scales a palette as what it is or not at all
  if (pal == WEED_PALETTE_RGBA32 || pal == WEED_PALETTE_BGRA32 || pal == WEED_PALETTE_YUVA8888) return WEED_PALETTE_RGBA32;
  if (pal == WEED_PALETTE_RGB24 || pal == WEED_PALETTE_BGR24 || pal == WEED_PALETTE_YUV888) return WEED_PALETTE_RGB24;
  if (pal == WEED_PALETTE_YVU420P) return WEED_PALETTE_YUV420P;
  return WEED_PALETTE_NONE;
}
static int inter_pal(int inpal, int outpal, bool upscale) {            // get_inter_pal (:14516-14575)
  const bool both_alpha = pal_has_alpha(inpal) && pal_has_alpha(outpal), any_planar = pal_is_planar_yuv(inpal) || pal_is_planar_yuv(outpal);
  const int rgb = both_alpha ? WEED_PALETTE_RGBA32 : WEED_PALETTE_RGB24;
  const int yuv = any_planar ? (both_alpha ? WEED_PALETTE_YUVA4444P : WEED_PALETTE_YUV444P) : (both_alpha ? WEED_PALETTE_YUVA8888 : WEED_PALETTE_YUV888);
  if (pal_is_rgb(inpal) && pal_is_rgb(outpal)) return rgb;
  if (pal_is_yuv(inpal) && pal_is_yuv(outpal)) return yuv;
  // rgb <-> yuv (or a hint that is neither: ANY): convert before an upscale, after a downscale
  if (pal_is_rgb(inpal)) return upscale ? yuv : rgb;
  return upscale ? rgb : yuv;
}
// get_resizable (:14577-14669).  LIVES_RESULT_SUCCESS = 1, LIVES_RESULT_FAIL = 0 (src/defs.h:211-212).  Where the reference ends in LIVES_FATAL ("Unable to
// convert from palette ...": neither the intermediate palette nor a masquerade of it is resizable) this returns FAIL with the arguments as they came.
int lives_gpu_get_resizable(int *ppalette, int *pxpal, int *oclamp_hint, int *opal, int *pxopal, lives_gpu_boolean upscale) {
  if (!ppalette || !opal) return 0;
  int resolved = WEED_PALETTE_NONE;
  const int palette = *ppalette;
  int xpalette = palette, opal_hint = *opal, xopal_hint = opal_hint;
  const bool in_resizable = pal_resizable(palette), out_resizable = pal_resizable(opal_hint);
  if (in_resizable) {
    if (opal_hint != WEED_PALETTE_ANY) {
      if (out_resizable) resolved = palette;
      else if (upscale) {
        const int omasq = masq_pal(opal_hint);
        if (omasq != WEED_PALETTE_NONE) { resolved = opal_hint; xpalette = xopal_hint = omasq; }
      }
    }
    if (resolved == WEED_PALETTE_NONE) resolved = xopal_hint = opal_hint = xpalette = palette;
  } else if (out_resizable) {
    if (!upscale || opal_hint == WEED_PALETTE_ANY) {
      const int imasq = masq_pal(palette);
      if (imasq) { resolved = opal_hint = palette; xpalette = xopal_hint = imasq; }
    }
    if (resolved == WEED_PALETTE_NONE) resolved = xpalette = xopal_hint = opal_hint;
  } else {
    int imasq = resolved = inter_pal(palette, opal_hint, upscale != 0);
    if (resolved == WEED_PALETTE_NONE || !pal_resizable(resolved)) {
      if (resolved != WEED_PALETTE_NONE) imasq = masq_pal(resolved);
      if (imasq == WEED_PALETTE_NONE) return 0;                        // LIVES_FATAL in the reference
    }
    opal_hint = resolved;
    xpalette = xopal_hint = imasq;
  }
  if (resolved == WEED_PALETTE_NONE) return 0;
  *ppalette = resolved;
  *opal = opal_hint;
  if (pxpal) *pxpal = xpalette;
  if (pxopal) *pxopal = xopal_hint;
  if (oclamp_hint && pal_is_yuv(resolved) && pal_is_rgb(xpalette)) *oclamp_hint = WEED_YUV_CLAMPING_UNCLAMPED;
  return 1;
}
int lives_gpu_get_tgt_gamma(int ipal, int opal) { return (pal_is_rgb(ipal) && pal_is_yuv(opal)) ? WEED_GAMMA_SRGB : WEED_GAMMA_UNKNOWN; }      // :14736-14740
// can_inline_gamma (:12128-12145) for the conversions of this library: a target gamma is folded into the conversion kernel for RGB <-> RGB (LUT8 in the
// swizzle), 4:2:0 / 4:2:2 planar -> RGB (the 16-bit LUT of :3274-3283) and RGB -> UYVY / YUYV; every other pair takes its gamma as a separate pass (the
// reference's rule answers TRUE for more pairs than its own conversions honour).
lives_gpu_boolean lives_gpu_can_inline_gamma(int inpl, int opal) {
  if (pal_is_rgb(inpl) && pal_is_rgb(opal)) return 1;
  if ((inpl == WEED_PALETTE_YUV420P || inpl == WEED_PALETTE_YVU420P || inpl == WEED_PALETTE_YUV422P) && pal_is_rgb(opal)) return 1;
  if (pal_is_rgb(inpl) && (opal == WEED_PALETTE_UYVY || opal == WEED_PALETTE_YUYV)) return 1;
  return 0;
}
// pconv_can_inplace (:12148-12157): TRUE where the conversion leaves the layer's pixel_data where it is.  Here every conversion writes new planes (the old ones go
// back through the host's allocator) except the byte swap between the two packed 4:2:2 orders; the planner books one more frame for the others (src/nodemodel.c:2961).
lives_gpu_boolean lives_gpu_pconv_can_inplace(int inpl, int outpl) {
  return (inpl == WEED_PALETTE_UYVY && outpl == WEED_PALETTE_YUYV) || (inpl == WEED_PALETTE_YUYV && outpl == WEED_PALETTE_UYVY);
}

// The gdk-pixbuf form of resize_layer_full (src/colourspace.c:14759-14937 + :15262-15322): the value it returns.
//   * size rules (:14854-14868): even source size only for the "nothing to do" test, width / height >= 4, even target height
//   * the palette resolution every build runs BEFORE its body (:14869-14912): get_resizable picks the palette the frame is scaled in -- a palette outside the body's
//     switch is first converted (to the hinted palette when that one is resizable, else to an intermediate one), with the target-gamma decision of :14890-14899
//     handed to that conversion; the call ends FALSE where the reference does: no resizable route (its LIVES_FATAL), or the layer does not have the resolved
//     palette / the hinted clamping afterwards (:14916-14923).  Quirk R2 (docs/QUIRKS.md): weed_layer_get_yuv_clamping() answers 0 = CLAMPED for a layer
//     without the leaf, which is every RGB layer, so an RGB frame with oclamp_hint UNCLAMPED fails that test -- as in the reference (unletterbox_layer :15628 passes
//     exactly that)
//   * clamped YUV888 / YUVA8888 is switched to unclamped inside the body (:15277-15284)
//   * the WHOLE layer (odd sizes included: the sizes are re-read at :15263-15264) is scaled; 4-byte palettes weight colours by alpha
//   * the new frame has the pixbuf's rowstride, ALIGN4(width * channels), and RGB layers come back tagged WEED_GAMMA_SRGB (pixbuf_to_layer :14378-14379,
//     :14405-14406), whatever they were tagged before; no gamma LUT runs in this body
static int width_pixels(const Layer &l) {       // weed_layer_get_width_pixels: the width leaf counts macropixels
  return (l.pal == WEED_PALETTE_UYVY || l.pal == WEED_PALETTE_YUYV) ? l.width * 2 : l.pal == WEED_PALETTE_YUV411 ? l.width * 4 : l.width;
}
// lgpu_pixbuf_scale_check with the calling thread's last positive answer remembered: the tracks of a render ask for the same geometry tick after tick, and
// sixteen host threads queueing for the scaler's table cache lock every tick is what the answer would otherwise cost
static bool scale_is_served(int sw, int sh, int dw, int dh, int interp) {
  thread_local int last[5] = {0, 0, 0, 0, -1};
  if (last[0] == sw && last[1] == sh && last[2] == dw && last[3] == dh && last[4] == interp) return true;
  if (lgpu_pixbuf_scale_check(sw, sh, dw, dh, 4, interp, S()) != LGPU_OK) return false;
  last[0] = sw; last[1] = sh; last[2] = dw; last[3] = dh; last[4] = interp;
  return true;
}
static int resize_pixbuf_body(weed_plant_t *layer, int width, int height, int interp, int opal_hint, int oclamp_hint, int osamp_hint, int osubs_hint, int tgt_gamma) {
  Layer l;
  if (!ready() || !read_layer(layer, &l)) return 0;
  if (opal_hint == WEED_PALETTE_NONE) opal_hint = WEED_PALETTE_ANY;                  // :14822
  if (width <= 0 || height <= 0) return 0;
  int iwidth = (width_pixels(l) >> 1) << 1, iheight = (l.height >> 1) << 1;
  if (width < 4) width = 4;
  if (height < 4) height = 4;
  if (iwidth != width || iheight != height) height = (height >> 1) << 1;
  if (iwidth == width && iheight == height) return 1;
  const int palette = l.pal;
  int iclamping = l.clamping < 0 ? 0 : l.clamping;                                   // weed_layer_get_yuv_clamping: 0 without the leaf
  int resolved = palette, xpalette, xopal_hint;
  const int upscale = (long)width * height > (long)iwidth * iheight;
  if (!lives_gpu_get_resizable(&resolved, &xpalette, &oclamp_hint, &opal_hint, &xopal_hint, upscale)) {
    fprintf(stderr, "Unable to convert from palette %d to palette %d\n", palette, opal_hint);
    return decline(layer);
  }
  if (tgt_gamma == WEED_GAMMA_UNKNOWN && pal_is_yuv(opal_hint) && osubs_hint == WEED_YUV_SUBSPACE_BT709) tgt_gamma = WEED_GAMMA_BT709;      // :14890-14899
  if (tgt_gamma == WEED_GAMMA_UNKNOWN) tgt_gamma = lives_gpu_get_tgt_gamma(palette, opal_hint);
  if (tgt_gamma == WEED_GAMMA_UNKNOWN) tgt_gamma = l.gamma;
  if (tgt_gamma == WEED_GAMMA_BT709 && pal_is_yuv(opal_hint)) osubs_hint = WEED_YUV_SUBSPACE_BT709;
  if (resolved != palette || oclamp_hint != iclamping) {
    lives_gpu_convert_layer_palette_full(layer, resolved, oclamp_hint, osamp_hint, osubs_hint, tgt_gamma);      // :14907 (its value is not looked at there either)
    if (!read_layer(layer, &l)) return 0;
  }
  iclamping = l.clamping < 0 ? 0 : l.clamping;
  if (l.pal != resolved || iclamping != oclamp_hint) return decline(layer);          // :14916-14923
  iwidth = (width_pixels(l) >> 1) << 1; iheight = (l.height >> 1) << 1;
  if (iwidth == width && iheight == height) return 1;
  // ---- the body (:15262-15322)
  if (width_pixels(l) == width && l.height == height) return 1;                     // "no resize needed" (:15265-15270) comes before the switch, for every palette
  if (!pal_is_pixbuf(l.pal) || (interp != LIVES_INTERP_FAST && interp != LIVES_INTERP_NORMAL && interp != LIVES_INTERP_BEST)) {
    if (!pal_is_pixbuf(l.pal)) fprintf(stderr, "Warning: resizing unknown palette %d\n", l.pal);
    fprintf(stderr, "unable to scale layer to %d x %d for palette %d\n", width, height, l.pal);
    return decline(layer);
  }
  if ((l.pal == WEED_PALETTE_YUV888 || l.pal == WEED_PALETTE_YUVA8888) && iclamping == WEED_YUV_CLAMPING_CLAMPED) {
    if (!lives_gpu_convert_layer_palette(layer, l.pal, WEED_YUV_CLAMPING_UNCLAMPED)) return 0;
    if (!read_layer(layer, &l)) return 0;
  }
  if (l.width == width && l.height == height) return 1;
  const int ch = (l.pal == WEED_PALETTE_RGB24 || l.pal == WEED_PALETTE_BGR24 || l.pal == WEED_PALETTE_YUV888) ? 3 : 4;
  if (lazy_pal(l.pal)) {
    // a pinned RGBA32 / BGRA32 frame: the scale is recorded (deferred execution) once the scaler has said it takes the geometry
    if (Lazy *z = lazy_detach(l, LZ_SCALE)) {
      if (scale_is_served(l.width, l.height, width, height, interp)) {
        const int prev = z->stage;
        z->scale = true; z->dw = width; z->dh = height; z->interp = interp; z->stage = LZ_SCALE; z->opaque = has_leaf(layer, kLeafOpaque) || z->yuv;      // a converted 4:2:0 frame has alpha 255 everywhere
        if (!lazy_commit(layer, l, z, l.pal, width, height, 4)) { z->scale = false; z->opaque = false; z->stage = prev; lazy_reattach(l.pd[0], z); return 0; }
        if (l.gamma != WEED_GAMMA_SRGB) set_int(layer, WEED_LEAF_GAMMA_TYPE, WEED_GAMMA_SRGB);
        return 1;
      }
      lazy_reattach(l.pd[0], z);          // the eager path below answers (and declines what the scaler does not cover)
    }
  }
  NewPlanes np;
  if (!alloc_planes(l.pal, width, height, 4, &np)) return 0;
  Work w;
  const uint8_t *d_in = w.in(l.pd[0], (size_t)l.rs[0] * l.height, 0);
  uint8_t *d_out = w.out(np.pd[0], (size_t)np.rs[0] * height, 3, np.rs[0] != width * ch);
  const int rc = w.ok ? lgpu_pixbuf_scale(d_in, l.rs[0], l.width, l.height, d_out, np.rs[0], width, height, ch, interp | ((ch == 4 && has_leaf(layer, kLeafOpaque)) ? LGPU_INTERP_OPAQUE : 0), S()) : LGPU_E_HIP;
  if (rc != LGPU_OK || !w.finish()) {
    drop_new_planes(np);
    return rc == LGPU_E_UNSUPPORTED ? decline(layer) : 0;      // reductions past the library's one-step range: the host's own body takes them
  }
  free_planes(l);
  commit_planes(layer, l.pal, width, height, np);
  if (pal_is_rgb(l.pal) && l.gamma != WEED_GAMMA_SRGB) set_int(layer, WEED_LEAF_GAMMA_TYPE, WEED_GAMMA_SRGB);
  return 1;
}

// resize_layer_full (src/colourspace.c:14759-15328).  PIXBUF backend: the reference's own sequence (palette resolution, pre-conversion, gdk-pixbuf body).
// POLYPHASE backend (the opt-in standing where the swscale body stands): the layer keeps its palette when the scaler takes it as it is (packed RGB, planar YUV;
// "layer palette should be checked on return", :14746-14751), a packed-YUV frame is first taken to the hinted palette, and osamp_hint / osubs_hint take part in
// the target-gamma decision only (:14890-14899).
static lives_gpu_boolean resize_layer_full(lives_gpu_layer_t *layer, int width, int height, int interp, int opal_hint, int oclamp_hint, int osamp_hint, int osubs_hint, int tgt_gamma) {
  if (g_resize_backend.load() == LIVES_GPU_RESIZE_PIXBUF) return resize_pixbuf_body(layer, width, height, interp, opal_hint, oclamp_hint, osamp_hint, osubs_hint, tgt_gamma);
  ResizePlan rp;
  int rc;
  if (plan_resize(layer, width, height, opal_hint, osubs_hint, tgt_gamma, &rp, &rc) != 1) return rc;
  NewPlanes np;
  if (!resize_into(rp.src, rp.width, rp.height, interp, 16, rp.use_lut ? rp.lut : nullptr, &np)) return 0;       // rowstride_alignment_hint = 16 (:14989)
  free_planes(rp.l);
  commit_planes(layer, rp.l.pal, rp.width, rp.height, np);
  if (rp.new_gamma != rp.l.gamma) set_int(layer, WEED_LEAF_GAMMA_TYPE, rp.new_gamma);
  return 1;
}
lives_gpu_boolean lives_gpu_resize_layer_full(lives_gpu_layer_t *layer, int width, int height, int interp, int opal_hint, int oclamp_hint,
                                              int osamp_hint, int osubs_hint, int tgt_gamma) {
  return pinned(layer, [&] { return resize_layer_full(layer, width, height, interp, opal_hint, oclamp_hint, osamp_hint, osubs_hint, tgt_gamma); });
}

lives_gpu_boolean lives_gpu_resize_layer(lives_gpu_layer_t *layer, int width, int height, int interp, int opal_hint, int oclamp_hint) {
  return lives_gpu_resize_layer_full(layer, width, height, interp, opal_hint, oclamp_hint, WEED_YUV_SAMPLING_DEFAULT,
                                     WEED_YUV_SUBSPACE_YCBCR, WEED_GAMMA_UNKNOWN);                        // :15331-15335
}

static lives_gpu_boolean letterbox_layer(lives_gpu_layer_t *layer, int nwidth, int nheight, int width, int height, int interp, int tpal, int tclamp) {
  if (!width || !height || !nwidth || !nheight) return 1;                 // :15377
  if (nwidth < width) nwidth = width;
  if (nheight < height) nheight = height;
  if (nheight == height && nwidth == width) { lives_gpu_resize_layer(layer, width, height, interp, tpal, tclamp); return 1; }
  // The inner frame: what resize_layer(layer, width, height, interp, tpal, tclamp) would leave (:15389) -- scaled STRAIGHT INTO the canvas when it has to
  // be scaled (the resized frame never exists on its own: one plane-sized write and read less per plane), blitted when it already has its size.
  ResizePlan rp;
  int rc, todo = 2;
  if (!ready() || !read_layer(layer, &rp.l)) return 0;
  if (g_resize_backend.load() == LIVES_GPU_RESIZE_PIXBUF && (width_pixels(rp.l) != width || rp.l.height != height)) {
    // the pixbuf body as the reference runs it: resize_layer first (:15389), then the blit of the frame it left
    if (!lives_gpu_resize_layer(layer, width, height, interp, tpal, tclamp)) return 0;
    if (!read_layer(layer, &rp.l)) return 0;
    width = rp.l.width; height = rp.l.height;
  }
  if (!(pal_is_rgb(rp.l.pal) || pal_is_planar_yuv(rp.l.pal)) && pal_psize(rp.l.pal) == 0) return decline(layer);   // packed YUV the blit has no pixel size for
  if (rp.l.width != width || rp.l.height != height) {                                     // resize_layer is only called for a frame of another size
    todo = plan_resize(layer, width, height, tpal, WEED_YUV_SUBSPACE_YUV, WEED_GAMMA_UNKNOWN, &rp, &rc);
    if (todo == 0) return rc;
  }
  const Layer &l = rp.l;
  Layer inner = l;                                       // the frame as it sits in the canvas
  if (todo == 1) { inner.width = rp.width; inner.height = rp.height; }
  width = inner.width; height = inner.height;
  if (nwidth < width || nheight < height) {              // cannot hold it (the reference asserts its sizes earlier): leave the layer resized, as the two calls did
    if (todo == 1) {
      NewPlanes rnp;
      if (!resize_into(rp.src, rp.width, rp.height, interp, 16, rp.use_lut ? rp.lut : nullptr, &rnp)) return 0;
      free_planes(l);
      commit_planes(layer, l.pal, rp.width, rp.height, rnp);
      if (rp.new_gamma != l.gamma) set_int(layer, WEED_LEAF_GAMMA_TYPE, rp.new_gamma);
    }
    return 0;
  }
  if (todo == 2 && lazy_pal(l.pal) && plane_is_lazy(l.pd[0])) {
    // the frame is a pending program (it has just been scaled): the canvas becomes its next stage
    if (Lazy *z = lazy_detach(l, LZ_CANVAS)) {
      const int prev = z->stage;
      z->canvas = true; z->nw = nwidth; z->nh = nheight; z->ox = (nwidth - width + 1) >> 1; z->oy = (nheight - height + 1) >> 1; z->stage = LZ_CANVAS;
      if (!lazy_commit(layer, l, z, l.pal, nwidth, nheight, 0)) { z->canvas = false; z->stage = prev; lazy_reattach(l.pd[0], z); return 0; }
      return 1;
    }
  }
  Layer canvas = inner;
  canvas.width = nwidth; canvas.height = nheight;
  NewPlanes np;
  if (!alloc_planes(l.pal, nwidth, nheight, 0, &np)) return 0;
  Work w;
  bool ok = true;
  const int offs_x = (nwidth - width + 1) >> 1, offs_y = (nheight - height + 1) >> 1;     // :15522-15523
  for (int p = 0; p < np.n && ok; p++) {
    const int ps = pal_is_planar_yuv(l.pal) ? 1 : pal_psize(l.pal);
    // chroma planes: offsets scaled by the plane ratio and truncated (:15553-15556)
    const int px = (plane_w(inner, p) == inner.width) ? offs_x : (int)(offs_x * 0.5), py = (plane_h(inner, p) == inner.height) ? offs_y : (int)(offs_y * 0.5);
    uint8_t black[4] = {0, 0, 0, 0};
    if (pal_is_planar_yuv(l.pal)) black[0] = (p == 0) ? (l.clamping == WEED_YUV_CLAMPING_UNCLAMPED ? 0 : 16) : 128;
    else if (pal_alpha_first(l.pal)) black[0] = 255;
    else if (pal_alpha_last(l.pal)) black[3] = 255;
    const int iw = plane_w(inner, p), ih = plane_h(inner, p), cw = plane_w(canvas, p), chh = plane_h(canvas, p);
    const Layer &from = todo == 1 ? rp.src : l;
    const int sw = plane_w(from, p), sh = plane_h(from, p);
    const uint8_t *d_in = w.in(l.pd[p], (size_t)l.rs[p] * plane_h(l, p), p == 3 ? 7 : p);
    uint8_t *d_out = w.out(np.pd[p], (size_t)np.rs[p] * chh, 3 + p, np.rs[p] != cw * ps);     // the canvas keeps its zeroed row padding (the kernels paint every pixel)
    if (!w.ok) { ok = false; break; }
    if (todo == 1)
      ok = lgpu_letterbox_bars(d_out, np.rs[p], cw, chh, ps, black, px, py, iw, ih, S()) == LGPU_OK &&
           lgpu_resize(d_in, l.rs[p], sw, sh, d_out + (size_t)py * np.rs[p] + (size_t)px * ps, np.rs[p], iw, ih, ps, interp, rp.use_lut ? rp.lut : nullptr, S()) == LGPU_OK;
    else
      ok = lgpu_letterbox_at(d_in, l.rs[p], sw, sh, d_out, np.rs[p], cw, chh, ps, black, px, py, S()) == LGPU_OK;
  }
  ok = ok && w.finish();
  if (!ok) { drop_new_planes(np); return 0; }
  free_planes(l);
  commit_planes(layer, l.pal, nwidth, nheight, np);
  if (todo == 1 && rp.new_gamma != l.gamma) set_int(layer, WEED_LEAF_GAMMA_TYPE, rp.new_gamma);
  return 1;
}
lives_gpu_boolean lives_gpu_letterbox_layer(lives_gpu_layer_t *layer, int nwidth, int nheight, int width, int height, int interp,
                                            int tpal, int tclamp) {
  return pinned(layer, [&] { return letterbox_layer(layer, nwidth, nheight, width, height, interp, tpal, tclamp); });
}

// unletterbox_layer (src/colourspace.c:15570-15628): cut the borders off, then resize to (opwidth, opheight) (0 = keep, -1 = the outer
// size).  Packed palettes only, as in the reference.  Quirk U1: the reference's row copy moves `xwidth` BYTES, not pixels
// (:15614), so only the first xwidth / psize pixels of every row arrive and the rest of the new (black, opaque) frame stays black: kept.
static lives_gpu_boolean unletterbox_layer(lives_gpu_layer_t *layer, int opwidth, int opheight, int top, int bottom, int left, int right) {
  Layer l;
  if (!layer || !ready() || !read_layer(layer, &l)) return 0;
  if (top < 0) top = 0;
  if (bottom < 0) bottom = 0;
  if (left < 0) left = 0;
  if (right < 0) right = 0;
  if (!pal_is_rgb(l.pal)) return decline(layer);
  const int width = l.width, height = l.height, ps = pal_psize(l.pal);
  const int xwidth = width - left - right, xheight = height - top - bottom;
  if ((xwidth == width && xheight == height) || xwidth <= 0 || xheight <= 0) return 1;
  NewPlanes np;
  if (!alloc_planes(l.pal, xwidth, xheight, 0, &np)) return 0;
  uint8_t black[4] = {0, 0, 0, 0};
  if (pal_alpha_first(l.pal)) black[0] = 255; else if (pal_alpha_last(l.pal)) black[3] = 255;
  {
    Work w;
    const uint8_t *d_in = w.in(l.pd[0], (size_t)l.rs[0] * height, 0);
    uint8_t *d_out = w.out(np.pd[0], np.sz[0], 3, true);
    // the copied part of a row is xwidth bytes = xwidth / ps whole pixels (+ xwidth % ps bytes of the next one: a byte-granular blit)
    const bool ok = w.ok && lgpu_fill_pattern(d_out, np.rs[0], black, ps, xwidth, xheight, S()) == LGPU_OK &&          // create_empty_pixel_data(black_fill)
                    lgpu_copy_rows(d_out, np.rs[0], d_in + (size_t)top * l.rs[0] + (size_t)left * ps, l.rs[0], xwidth, xheight, S()) == LGPU_OK && w.finish();
    if (!ok) { drop_new_planes(np); return 0; }
  }
  free_planes(l);
  commit_planes(layer, l.pal, xwidth, xheight, np);
  if (opwidth == -1) opwidth = width; else if (!opwidth) opwidth = xwidth;
  if (opheight == -1) opheight = height; else if (!opheight) opheight = xheight;
  if (opwidth == xwidth && opheight == xheight) return 1;
  return lives_gpu_resize_layer(layer, opwidth, opheight, LIVES_INTERP_BEST, WEED_PALETTE_ANY, WEED_YUV_CLAMPING_UNCLAMPED);
}
lives_gpu_boolean lives_gpu_unletterbox_layer(lives_gpu_layer_t *layer, int opwidth, int opheight, int top, int bottom, int left, int right) {
  return pinned(layer, [&] { return unletterbox_layer(layer, opwidth, opheight, top, bottom, left, right); });
}

// compact_rowstrides (src/colourspace.c:14439-14496): new pixel data whose rowstrides are exactly width * bytes per (macro)pixel * plane ratio
static lives_gpu_boolean compact_rowstrides(lives_gpu_layer_t *layer) {
  Layer l;
  if (!ready() || !read_layer(layer, &l)) return 0;
  int bpm = pal_psize(l.pal);                                               // bytes per macropixel of plane 0
  if (l.pal == WEED_PALETTE_UYVY || l.pal == WEED_PALETTE_YUYV || l.pal == WEED_PALETTE_YUVA8888) bpm = 4;
  else if (l.pal == WEED_PALETTE_YUV888) bpm = 3;
  else if (l.pal == WEED_PALETTE_YUV411) bpm = 6;
  if (!bpm) return decline(layer);
  NewPlanes np;
  np.n = l.nplanes;
  bool change = false;
  size_t tot = 0;
  for (int p = 0; p < l.nplanes; p++) {
    np.rs[p] = plane_w(l, p) * bpm;
    np.sz[p] = (size_t)np.rs[p] * plane_h(l, p);
    tot += np.sz[p];
    if (np.rs[p] != l.rs[p]) change = true;
  }
  if (!change) return 1;
  uint8_t *blk = (uint8_t *)palloc(tot + 64, false);
  if (!blk) return 0;
  memset(blk + tot, 0, 64);
  size_t off = 0;
  for (int p = 0; p < np.n; p++) { np.pd[p] = blk + off; off += np.sz[p]; }
  {
    Work w;
    bool ok = true;
    for (int p = 0; p < np.n && ok; p++) {
      const uint8_t *d_in = w.in(l.pd[p], (size_t)l.rs[p] * plane_h(l, p), p == 3 ? 7 : p);
      uint8_t *d_out = w.out(np.pd[p], np.sz[p], 3 + p, false);
      ok = w.ok && lgpu_copy_rows(d_out, np.rs[p], d_in, l.rs[p], np.rs[p], plane_h(l, p), S()) == LGPU_OK;
    }
    if (!ok || !w.finish()) { pfree(blk); return 0; }
  }
  free_planes(l);
  commit_planes(layer, l.pal, l.width, l.height, np);
  return 1;
}
lives_gpu_boolean lives_gpu_compact_rowstrides(lives_gpu_layer_t *layer) {
  return pinned(layer, [&] { return compact_rowstrides(layer); });
}

// weed_layer_clear_pixel_data (src/colourspace.c:11229-11244): the frame painted black in place (blank_frame :11212-11226): host
// bytes of an ordinary layer (a fill of host memory is the host's business), the resident planes of a pinned one.  Packed palettes
// keep the reference's per-pixel pattern (opaque alpha); YUYV keeps its quirk (blank_pixel :11150-11154 never advances: only the first
// macropixel of a row is written).
static lives_gpu_boolean weed_layer_clear_pixel_data(lives_gpu_layer_t *layer) {
  Layer l;
  if (!layer || !bound() || !read_layer(layer, &l)) return 0;
  const int clamping = l.clamping >= 0 ? l.clamping : WEED_YUV_CLAMPING_CLAMPED;       // weed_layer_get_palette_yuv: CLAMPED when the leaf is missing
  const uint8_t yb = clamping == WEED_YUV_CLAMPING_UNCLAMPED ? 0 : 16;
  uint8_t pat[8];
  int plen = 0, nmp = l.width;                    // pattern of one (macro)pixel of plane 0, macropixels per row
  switch (l.pal) {
  case WEED_PALETTE_RGB24: case WEED_PALETTE_BGR24: pat[0] = pat[1] = pat[2] = 0; plen = 3; break;
  case WEED_PALETTE_RGBA32: case WEED_PALETTE_BGRA32: pat[0] = pat[1] = pat[2] = 0; pat[3] = 255; plen = 4; break;
  case WEED_PALETTE_ARGB32: pat[0] = 255; pat[1] = pat[2] = pat[3] = 0; plen = 4; break;
  case WEED_PALETTE_UYVY: pat[0] = pat[2] = 128; pat[1] = pat[3] = yb; plen = 4; break;
  case WEED_PALETTE_YUYV: pat[0] = pat[2] = yb; pat[1] = pat[3] = 128; plen = 4; nmp = 1; break;
  case WEED_PALETTE_YUV888: pat[0] = yb; pat[1] = pat[2] = 128; plen = 3; break;
  case WEED_PALETTE_YUVA8888: pat[0] = yb; pat[1] = pat[2] = 128; pat[3] = 255; plen = 4; break;
  case WEED_PALETTE_YUV411: pat[0] = pat[3] = 128; pat[1] = pat[2] = pat[4] = pat[5] = yb; plen = 6; break;
  default: break;
  }
  if (!plen && !pal_is_planar_yuv(l.pal)) return 0;
  const bool on_device = t_pinned && ready();
  for (int p = 0; p < l.nplanes; p++) {
    const int ph = plane_h(l, p), pw = plane_w(l, p);
    uint8_t one[1] = {(uint8_t)(p == 0 ? yb : p == 3 ? 255 : 128)};
    const uint8_t *pp = plen ? pat : one;
    const int pl = plen ? plen : 1, n = plen ? nmp : pw;
    uint8_t *d = on_device ? resident(l.pd[p], (size_t)l.rs[p] * ph, true) : nullptr;
    if (d) {
      const int rc = lgpu_fill_pattern(d, l.rs[p], pp, pl, n, ph, S());
      touch_done(l.pd[p], true);
      if (rc != LGPU_OK) return 0;
      continue;
    }
    for (int y = 0; y < ph; y++) {
      uint8_t *row = l.pd[p] + (size_t)y * l.rs[p];
      if (pl == 1) memset(row, pp[0], (size_t)n);
      else for (int x = 0; x < n; x++) memcpy(row + (size_t)x * pl, pp, (size_t)pl);
    }
  }
  return 1;
}
lives_gpu_boolean lives_gpu_weed_layer_clear_pixel_data(lives_gpu_layer_t *layer) {
  return pinned(layer, [&] { return weed_layer_clear_pixel_data(layer); });
}

// The host's word that every pixel of the layer's frame has alpha 255 (decoded video, a frame that was RGB24 / YUV before): the scalers then run their all-opaque
// instantiations (LGPU_INTERP_OPAQUE: same bytes on such frames, 25-30 % less time for enlargements).  The word is the host's to keep true: it stays on the layer
// through the seam's own calls (a scale, letterbox, R <-> B, gamma or chroma blend of an opaque frame is opaque) until the host takes it back (on = 0) or hands
// the layer a new frame.  A frame that is not opaque gets wrong colours.
int lives_gpu_layer_set_opaque(lives_gpu_layer_t *layer, int on) {
  if (!layer || !bound()) return LGPU_E_BADARG;
  if (on) set_int(layer, kLeafOpaque, 1);
  else if (has_leaf(layer, kLeafOpaque)) g_api.leaf_delete(layer, kLeafOpaque);
  return LGPU_OK;
}
}  // extern "C"
