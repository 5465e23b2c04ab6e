// flat_select.hip -- a SELECT transition between two decoded frames in one launch (lgpu_chain_flat_yuv_select, include/lives_gpu_select.h): iris rectangle, iris circle
// and dissolve of multi_transitions.c on two YUV420P / YUV422P / UYVY / YUYV layers:
// conversion of the SHOWN layer -> [R <-> B] [-> letterbox onto opaque black] -> select [-> gamma LUT] -> RGBA, or -> K4's conversion to UYVY / YUYV / YUV420P.
//
// flat.hip's mix forms convert both layers at every cell, because a crossfade needs both.  A select does not: which layer a pixel shows is known from its coordinates,
// the track's amount and (dissolve) its mask value before anything is loaded.  A lane owns the cell (unit, k) of flat.hip's unit walk -- two pixels of one row or a
// 2 x 2 quad.  It first evaluates the predicate (select_pred.h, the one k_transition and k_dissolve take) for its two or four pixels; then each layer's loads and walk
// (flat_walk.h, the functions k_flat_yuv420 calls) run under a WAVE-UNIFORM condition, a vote over the wave: layer 2's only if some lane of the wave shows a layer-2
// pixel, layer 1's only if some lane shows a layer-1 pixel.  A wave wholly inside or wholly outside the figure issues no load of the hidden layer's planes and none
// of its table gathers; at amount 0 or 1 no wave of the launch does.  Waves on the outline, and every wave of a dissolve strictly between 0 and 1, convert both and
// select per pixel.  The finished pixel takes flat.hip's path: LUT, store or K4; the 4:2:0 sink's chroma comes from whichever layers' pixels the row pair shows.
//
// The figure is the CANVAS's where there is one: the predicate takes (x + offs_x, y + offs_y) in an nwidth x nheight frame of 4-byte pixels, the dissolve mask is
// nwidth * nheight floats, and the bars are select(black, black) = opaque black [-> LUT], written by the same launch with nothing read for them.
//
// Per-track data: the four values the amount decides (TransAmt, derived by effects.hip's transition_amount as for lgpu_transition) and the mask pointer travel in the
// kernel arguments with the nine plane pointers: 32 tracks per launch (LGPU_CHAIN_SELECT_TRACKS; 64 would not fit HIP's 4 KB), 33..64 as two launches on the stream.
#include "lgpu_common.h"
#include "../../include/lives_gpu_select.h"
#include "k2_walk.h"
#include "flat_walk.h"
#include "select_pred.h"
#include <algorithm>
#include <cmath>
#include <string.h>

namespace lgpu { int cavg_forms_checked(); }      // palette.hip
int get_sink_tables(int which_tables, int in_order, const uint2 **out);      // pixbuf.hip

namespace lgpu {

struct SelLayer {
  const int32_t *tables;         // device [5][256] RGB_Y R_Cr G_Cb G_Cr B_Cb (layer 2: null when layer 1's staged copy serves both)
  uint32_t usize, vsize;         // chroma plane bytes; K2's read one past the last row's end is clamped to the last byte of THIS layer's plane
  int ys, us, vs;
  int clamped, lowq, fix_edges;
  int sfmt;                      // packed: 2 UYVY, 3 YUYV (wave-uniform)
};
struct SelArgs {
  SelLayer l1, l2;
  const uint2 *stab;             // sink: device [2][3][256] (get_sink_tables)
  int w, h;                      // the frame
  int orow, urow, vrow;          // destination (RGBA / packed / luma) and 4:2:0 chroma rowstrides
  int cw, ch, ox, oy;            // canvas (cw == 0: none)
  int use_lut, fmt, unclamped;   // sink: 2 UYVY, 3 YUYV, 4 YUV420P
  int gy_units, per;             // blockIdx.y < gy_units: the workgroup walks units [y * per, (y + 1) * per); the others write the canvas's bars
  int kind;                      // 0 iris rectangle, 1 iris circle, 3 dissolve (wave-uniform)
  int fw, fh;                    // the figure's frame: the canvas, or the frame without one
  int wb, ihwidth, ihheight;     // 4 * fw, and the figure's centre (TransGeom)
};
template <int NDST> struct SelTracksT {
  const uint8_t *y[LGPU_CHAIN_SELECT_TRACKS], *u[LGPU_CHAIN_SELECT_TRACKS], *v[LGPU_CHAIN_SELECT_TRACKS];
  const uint8_t *y2[LGPU_CHAIN_SELECT_TRACKS], *u2[LGPU_CHAIN_SELECT_TRACKS], *v2[LGPU_CHAIN_SELECT_TRACKS];
  uint8_t *dst[NDST][LGPU_CHAIN_SELECT_TRACKS];
  const float *mask[LGPU_CHAIN_SELECT_TRACKS];      // dissolve: (fw * fh) floats
  TransAmt amt[LGPU_CHAIN_SELECT_TRACKS];           // what the track's amount decides: xx, yy (rectangle), uthr (circle), bf (dissolve)
};
template <int SINK> struct SelSinkLds { uint2 t[6 * 256]; };
template <> struct SelSinkLds<0> {};
static_assert(sizeof(SelArgs) + sizeof(SelTracksT<1>) + sizeof(Lut8) <= 4096 && sizeof(SelArgs) + sizeof(SelTracksT<3>) + sizeof(Lut8) <= 4096,
              "HIP documents 4 KB of arguments for a __global__ function");

// SINK: 0 RGBA, 1 packed 4:2:2 (UYVY / YUYV), 2 planar 4:2:0.  SWAP: the finished pixel is BGRA (src->out_order ^ params->swap_rb), on both layers.
// SRC / SRC2: each layer's walk -- 0 planar 4:2:0, 1 planar 4:2:2 (YUV422P), 2 packed 4:2:2 (UYVY / YUYV; T.y / T.y2 is the frame, the chroma pointers are not read)
template <int SWAP, int SINK, int SRC, int SRC2>
__global__ __launch_bounds__(256) void k_flat_select(const SelArgs A, const SelTracksT<SINK == 2 ? 3 : 1> T, const Lut8 lut) {
  static_assert(SRC >= 0 && SRC <= 2 && SRC2 >= 0 && SRC2 <= 2 && SINK >= 0 && SINK <= 2, "SRC / SRC2: 0 4:2:0, 1 YUV422P, 2 packed");
  __shared__ uint32_t s_ty[2][256];
  __shared__ uint2 s_rg[2][256], s_gb[2][256];
  __shared__ __attribute__((aligned(16))) uint8_t s_lut[256];
  __shared__ SelSinkLds<SINK> s_sink;
  const int tid = threadIdx.x, z = blockIdx.z;
  stage_lut(s_lut, lut);
  if constexpr (SINK == 0) {
    if ((int)blockIdx.y >= A.gy_units) {
      // letterbox bars: both layers are letterboxed onto the same black canvas, so a bar pixel is select(black, black) = opaque black [-> LUT]; nothing is read
      __syncthreads();
      const int bb = ((int)blockIdx.y - A.gy_units) * (int)gridDim.x + (int)blockIdx.x, nbb = ((int)gridDim.y - A.gy_units) * (int)gridDim.x;
      const int top = A.oy * A.cw, bottom = (A.ch - A.oy - A.h) * A.cw, sw_ = A.cw - A.w, total = top + bottom + A.h * sw_;
      uint32_t c = 0xFF000000u;
      if (A.use_lut) c = lut3_rgba(s_lut, c);
      for (long p = (long)bb * 256 + tid; p < total; p += (long)nbb * 256) {
        int q = (int)p, x, y;
        if (q < top) { y = q / A.cw; x = q - y * A.cw; }
        else if (q < top + bottom) { q -= top; y = q / A.cw; x = q - y * A.cw; y += A.oy + A.h; }
        else { q -= top + bottom; y = q / sw_; x = q - y * sw_; y += A.oy; if (x >= A.ox) x += A.w; }
        reinterpret_cast<uint32_t *>(T.dst[0][z] + (size_t)y * A.orow)[x] = c;
      }
      return;
    }
  }
  {
    // K2's tables, paired, as k_flat_yuv420 stages them: the entry of an UNCLAMPED chroma value e is tables[clamp(e)].  Layer 2's own copy when its table set or its
    // index clamp differs (a packed layer indexes with the sample itself)
    auto stage = [&](int s, const SelLayer &L) {
      const int clo = L.clamped ? 16 : 0, chi = L.clamped ? 240 : 255;
      const int ec = tid < clo ? clo : tid > chi ? chi : tid;
      s_ty[s][tid] = (uint32_t)L.tables[tid];
      s_rg[s][tid] = make_uint2((uint32_t)L.tables[256 + ec], (uint32_t)L.tables[768 + ec]);
      s_gb[s][tid] = make_uint2((uint32_t)L.tables[512 + ec], (uint32_t)L.tables[1024 + ec]);
    };
    stage(0, A.l1);
    if (A.l2.tables) stage(1, A.l2);
    if constexpr (SINK != 0) {
#pragma unroll
      for (int i = 0; i < 6; i++) s_sink.t[tid + 256 * i] = A.stab[tid + 256 * i];
    }
  }
  __syncthreads();
  const int hw = A.w >> 1, H = A.h;
  const int k = (int)blockIdx.x * 256 + tid;
  if (k >= hw) return;           // the votes below are over the lanes that own a cell
  const int npairs = (H - 1) / 2;                            // full row pairs starting at row 1
  const int nunits = 1 + npairs + (((H - 1) & 1) ? 1 : 0);
  const FlatPlanes P1 = {T.y[z], T.u[z], T.v[z], A.l1.usize, A.l1.vsize, A.l1.ys, A.l1.us, A.l1.vs, A.l1.lowq, A.l1.fix_edges};
  const FlatPlanes P2 = {T.y2[z], T.u2[z], T.v2[z], A.l2.usize, A.l2.vsize, A.l2.ys, A.l2.us, A.l2.vs, A.l2.lowq, A.l2.fix_edges};
  const int own = A.l2.tables != nullptr;      // wave-uniform
  const FlatK2Lds L1 = {s_ty[0], s_rg[0], s_gb[0]}, L2 = {s_ty[own], s_rg[own], s_gb[own]};
  const TransAmt am = T.amt[z];
  const float *mask = T.mask[z];
  // does pixel (row i, column x) of the frame show layer 2?  The figure is computed on the canvas where there is one: 4-byte pixels, byte columns j = 4 x
  auto shows2 = [&](int i, int x) -> bool {
    const int fi = i + A.oy, fx = x + A.ox;
    if (A.kind == 0) return !LGPU_IRIS_RECT_SHOWS1(fi, 4 * fx, am.xx, am.yy, A.wb, A.fh);
    if (A.kind == 1) return !LGPU_IRIS_CIRCLE_SHOWS1(4, fi, 4 * fx, A.ihwidth, A.ihheight, am.uthr);
    return LGPU_DISSOLVE_SHOWS2(mask, A.fw, fi, fx, am.bf);
  };
  // the rest of the chain on the two finished pixels of frame row i, then the store (k_flat_yuv420's emit behind its blend); cu / cv: the clamped U of the first
  // pixel and V of the second (4:2:0 sink)
  auto emit = [&](int i, uint32_t p0, uint32_t p1, int &cu, int &cv) __attribute__((always_inline)) {
    if (A.use_lut) { p0 = lut3_rgba(s_lut, p0); p1 = lut3_rgba(s_lut, p1); }
    if constexpr (SINK == 0) {
      uint8_t *d = T.dst[0][z] + (size_t)(i + A.oy) * A.orow + 4 * (size_t)(2 * k + A.ox);
      if (multiple_of(reinterpret_cast<uintptr_t>(d), 8)) *reinterpret_cast<uint2 *>(d) = make_uint2(p0, p1);
      else { reinterpret_cast<uint32_t *>(d)[0] = p0; reinterpret_cast<uint32_t *>(d)[1] = p1; }
    } else {
      uint32_t y0c, y1c;
      int ur, vr;
      flat_k4_pair(s_sink.t, A.unclamped, p0, p1, y0c, y1c, ur, vr);
      const int min_uv = A.unclamped ? 0 : 16, max_uv = A.unclamped ? 255 : 240;
      if constexpr (SINK == 1) {
        // rgb2yuyv lost its `else`: only the lower chroma clamp, then the byte cast (src/colourspace.c:2183-2191)
        const int ul = max(ur, min_uv), vl = max(vr, min_uv);
        const uint32_t uu = (uint32_t)(A.fmt == 3 ? ul : min(ul, max_uv)) & 0xFFu, vv = (uint32_t)(A.fmt == 3 ? vl : min(vl, max_uv)) & 0xFFu;
        const uint32_t w = A.fmt == 3 ? (y0c | (uu << 8) | (y1c << 16) | (vv << 24)) : (uu | (y0c << 8) | (vv << 16) | (y1c << 24));
        reinterpret_cast<uint32_t *>(T.dst[0][z] + (size_t)i * A.orow)[k] = w;
      } else {
        reinterpret_cast<uint16_t *>(T.dst[0][z] + (size_t)i * A.orow)[k] = (uint16_t)(y0c | (y1c << 8));
        cu = min(max(ur, min_uv), max_uv); cv = min(max(vr, min_uv), max_uv);
      }
    }
  };
  const int u_lo = (int)blockIdx.y * A.per, u_hi = min(nunits, u_lo + A.per);
  for (int unit = u_lo; unit < u_hi; unit++) {
    // decide first: the cell's rows, and which layer each of its two or four pixels shows
    const bool pair = unit >= 1 && unit <= npairs;
    const int i = unit == 0 ? 0 : pair ? 2 * unit - 1 : H - 1;
    const bool s0 = shows2(i, 2 * k), s1 = shows2(i, 2 * k + 1);
    const bool s2 = pair ? shows2(i + 1, 2 * k) : s0, s3 = pair ? shows2(i + 1, 2 * k + 1) : s1;
    const bool some2 = __any((int)(s0 | s1 | s2 | s3)) != 0, some1 = __any((int)!(s0 & s1 & s2 & s3)) != 0;      // wave-uniform
    // SWAP | 2: the walks pack their pixels with byte permutes here (flat_walk.h, flat_px: the compiler's v_ashr_pk_u8_i32 behind the selects below)
    uint32_t p[4] = {0u, 0u, 0u, 0u}, q[4] = {0u, 0u, 0u, 0u};
    if (some2) {
      auto keep = [&](auto, int, int, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) __attribute__((always_inline)) { q[0] = a0; q[1] = a1; q[2] = b0; q[3] = b1; };
      if constexpr (SRC2 == 0) flat_cell<SWAP | 2>(P2, L2, unit, k, hw, H, npairs, keep);
      else flat_cell422<SWAP | 2, SRC2>(P2, L2, A.l2.sfmt, unit, k, H, npairs, keep);
    }
    if (some1) {
      auto keep = [&](auto, int, int, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) __attribute__((always_inline)) { p[0] = a0; p[1] = a1; p[2] = b0; p[3] = b1; };
      if constexpr (SRC == 0) flat_cell<SWAP | 2>(P1, L1, unit, k, hw, H, npairs, keep);
      else flat_cell422<SWAP | 2, SRC>(P1, L1, A.l1.sfmt, unit, k, H, npairs, keep);
    }
    int cu0 = 0, cv0 = 0, cu1 = 0, cv1 = 0;
    emit(i, s0 ? q[0] : p[0], s1 ? q[1] : p[1], cu0, cv0);       // row 0's chroma is never kept
    if (pair) {
      emit(i + 1, s2 ? q[2] : p[2], s3 ? q[3] : p[3], cu1, cv1);
      if constexpr (SINK == 2) {      // chroma row r = cavg(row 2r + 2, row 2r + 1): the argument order of the reference
        const int cl = !A.unclamped, r = unit - 1;
        T.dst[1][z][(size_t)r * A.urow + k] = (uint8_t)cavg_arith(cl, cu1, cu0);
        T.dst[2][z][(size_t)r * A.vrow + k] = (uint8_t)cavg_arith(cl, cv1, cv0);
      }
    } else if (unit != 0) {
      if constexpr (SINK == 2) {      // the trailing row of an even height: the last chroma row is row dh - 1's alone
        const int r = (H - 1) >> 1;
        T.dst[1][z][(size_t)r * A.urow + k] = (uint8_t)cu0;
        T.dst[2][z][(size_t)r * A.vrow + k] = (uint8_t)cv0;
      }
    }
  }
}

}  // namespace lgpu

using namespace lgpu;

// lgpu_chain_flat_yuv_select (include/lives_gpu_select.h): the checks are the mix form's -- check_yuv_source, check_yuv_sink, check_rgba_dest, check_track,
// check_plane_sizes (lgpu_common.h), its alignment rules and its order: LGPU_E_BADARG before LGPU_E_UNSUPPORTED, everything before anything is allocated or enqueued
extern "C" int lgpu_chain_flat_yuv_select(const lgpu_chain_params *pr, const lgpu_yuv_layer_source *s1, const lgpu_yuv_layer_source *s2, const lgpu_select *sel,
                                          const lgpu_canvas *cv, const lgpu_chain_sink *sk, const lgpu_chain_yuv_mix_track *tracks, int ntracks, void *stream) {
  static const char fn[] = "lgpu_chain_flat_yuv_select";
  int rc = ensure_init();
  if (rc) return rc;
#define SEL_REQUIRE(cond, msg) do { if (!(cond)) { set_error("%s: %s", fn, msg); return LGPU_E_BADARG; } } while (0)
#define SEL_REFUSE(msg) do { set_error("%s: %s", fn, msg); return LGPU_E_UNSUPPORTED; } while (0)
  SEL_REQUIRE(pr && s1 && s2 && sel && tracks && ntracks > 0 && ntracks <= LGPU_CHAIN_MAX_TRACKS, "params, both sources, the select and 1..64 tracks required");
  SEL_REQUIRE(s1->in_fmt >= 2 && s1->in_fmt <= 5 && s2->in_fmt >= 2 && s2->in_fmt <= 5, "in_fmt must be 2 (UYVY), 3 (YUYV), 4 (YUV420P) or 5 (YUV422P) on either layer");
  SEL_REQUIRE(!(cv && sk), "a canvas and a sink together: chroma rows would straddle the bar / frame edge");
  SEL_REQUIRE(pr->interp & LGPU_INTERP_PIXBUF, "the gdk-pixbuf arithmetic only (LGPU_INTERP_PIXBUF)");
  const int kind = sel->kind;
  SEL_REQUIRE(kind == LGPU_SELECT_IRIS_RECT || kind == LGPU_SELECT_IRIS_CIRCLE || kind == LGPU_SELECT_DISSOLVE,
              "kind must be 0 (iris rectangle), 1 (iris circle) or 3 (dissolve); the other transitions show layer 1 at a shifted position or need both layers");
  SEL_REQUIRE(sel->amounts, "null amounts");
  for (int i = 0; i < ntracks; i++) SEL_REQUIRE(std::isfinite(sel->amounts[i]) && sel->amounts[i] >= 0. && sel->amounts[i] <= 1., "a transition amount is a finite number in 0..1");
  if (kind == LGPU_SELECT_DISSOLVE) {
    SEL_REQUIRE(sel->mask_d, "dissolve needs the table of mask pointers");
    for (int i = 0; i < ntracks; i++) {
      SEL_REQUIRE(sel->mask_d[i], "null dissolve mask");
      SEL_REQUIRE(multiple_of((uintptr_t)sel->mask_d[i], 4), "a dissolve mask is read as floats (address % 4 == 0)");
    }
  }
  // one layer's description as the shared checks read it; what a packed layer does not have is zero
  auto source_of = [](const lgpu_yuv_layer_source *s) {
    lgpu_yuv_source ys;
    memset(&ys, 0, sizeof ys);
    const bool packed = s->in_fmt < 4;
    ys.istrides[0] = s->istrides[0]; ys.istrides[1] = packed ? 0 : s->istrides[1]; ys.istrides[2] = packed ? 0 : s->istrides[2];
    ys.u_size = packed ? 0 : s->u_size; ys.v_size = packed ? 0 : s->v_size;
    ys.out_order = s->out_order; ys.which_tables = s->which_tables; ys.pb_quality = s->pb_quality; ys.flags = s->flags;
    return ys;
  };
  const lgpu_yuv_source ys = source_of(s1), ys2 = source_of(s2);
  const bool packed1 = s1->in_fmt < 4, packed2 = s2->in_fmt < 4;
  const int srcp = packed1 ? 2 : s1->in_fmt == 5 ? 1 : 0, srcp2 = packed2 ? 2 : s2->in_fmt == 5 ? 1 : 0;      // the kernel's SRC / SRC2 policies
  if ((rc = check_yuv_source(fn, pr, &ys, s1->in_fmt)) || (rc = check_yuv_source(fn, pr, &ys2, s2->in_fmt))) return rc;
  const int chain_order = (ys.out_order ^ (pr->swap_rb ? 1 : 0)) & 1;
  SEL_REQUIRE(ys2.out_order == chain_order, "src2->out_order must state the byte order the select works in: src->out_order ^ params->swap_rb");
  const bool planar = sk && sk->out_fmt >= 4;
  const int nplanes = planar ? 3 : 1;
  if ((rc = sk ? check_yuv_sink(fn, pr, sk, chain_order, false) : check_rgba_dest(fn, pr, cv, false))) return rc;
  const int fw = cv ? cv->nwidth : pr->dw, fh = cv ? cv->nheight : pr->dh;      // the figure's frame, and the RGBA destination's
  uintptr_t pb = 0, sb = 0, sb2 = 0;
  for (int i = 0; i < ntracks; i++) {
    const lgpu_chain_yuv_mix_track &t = tracks[i];
    // a packed layer is its y plane alone: its chroma pointers are not read, so they may be null and are no plane a destination could collide with
    const uint8_t *const planes[3] = {t.y_d, packed1 ? nullptr : t.u_d, packed1 ? nullptr : t.v_d};
    const uint8_t *const u2 = packed2 ? nullptr : t.u2_d, *const v2 = packed2 ? nullptr : t.v2_d;
    if ((rc = check_track(fn, planes, packed1 ? 1 : 3, false, nullptr, false, t.dst_d, nplanes, !sk))) return rc;
    SEL_REQUIRE(t.y2_d && (packed2 || (u2 && v2)), "null layer-2 plane");
    for (int k = 0; k < nplanes; k++)
      SEL_REQUIRE((const uint8_t *)t.dst_d[k] != t.y2_d && (const uint8_t *)t.dst_d[k] != u2 && (const uint8_t *)t.dst_d[k] != v2, "a destination plane is one of layer 2's planes");
    sb |= (uintptr_t)t.y_d; sb2 |= (uintptr_t)t.y2_d; pb |= (uintptr_t)t.dst_d[0];
  }
  // the one-launch form; anything else is refused, never run some other way
  if (pr->sw != pr->dw || pr->sh != pr->dh) SEL_REFUSE("frames that keep their size only (sw == dw, sh == dh)");
  if (pr->do_blur) SEL_REFUSE("the gaussian is not offered with a 4:2:0 or 4:2:2 source");
  // K3 reads a macropixel as one aligned dword; the reference divides that rowstride by 4 (docs/QUIRKS.md, K3-c): there is no behaviour to follow elsewhere
  if (packed1 && !multiple_of(sb | (uintptr_t)ys.istrides[0], 4)) SEL_REFUSE("a UYVY / YUYV source is read as 4-byte macropixels (plane and rowstride % 4 == 0)");
  if (packed2 && !multiple_of(sb2 | (uintptr_t)ys2.istrides[0], 4)) SEL_REFUSE("a UYVY / YUYV layer 2 is read as 4-byte macropixels (plane and rowstride % 4 == 0)");
  if (sk) {
    if (sk->out_fmt == 5) SEL_REFUSE("YUV422P is not served (the RGBA form + lgpu_rgb_to_yuv_batch)");
    if (planar && (pr->dh & 1)) SEL_REFUSE("the 4:2:0 sink needs an even height");
    // a lane stores one macropixel (4 bytes) or one luma pair (2 bytes) per row; chroma samples are single bytes
    if (!multiple_of(pb | (uintptr_t)sk->orow[0], planar ? 2 : 4))
      SEL_REFUSE("packed sinks are stored as 4-byte macropixels (plane and rowstride % 4 == 0), the 4:2:0 luma plane as 2-byte pairs (plane and rowstride % 2 == 0)");
  }
  const int drow = sk ? sk->orow[0] : pr->orow;
  if ((rc = check_plane_sizes(fn, {(long long)pr->sh * ys.istrides[0], ys.u_size, ys.v_size, (long long)fh * drow, (long long)pr->sh * ys2.istrides[0], ys2.u_size, ys2.v_size,
                                   planar ? (long long)(pr->dh >> 1) * sk->orow[1] : 0, planar ? (long long)(pr->dh >> 1) * sk->orow[2] : 0}))) return rc;
  SelArgs a;
  memset(&a, 0, sizeof a);
  if (planar && (rc = cavg_forms_checked())) return rc;
  if (sk && (rc = get_sink_tables(sk->which_tables, sk->in_order, &a.stab))) return rc;
  auto layer_of = [](const lgpu_yuv_source &y, bool packed, int in_fmt) {
    SelLayer L;
    L.tables = device_tables()->yuv2rgb[y.which_tables & 3];
    L.usize = (uint32_t)y.u_size; L.vsize = (uint32_t)y.v_size; L.ys = y.istrides[0]; L.us = y.istrides[1]; L.vs = y.istrides[2];
    L.clamped = !packed && !(y.which_tables & 1);      // K3 indexes its tables with the sample itself
    L.lowq = y.pb_quality == 1; L.fix_edges = (y.flags & LGPU_YUV_FIX_EDGES) ? 1 : 0; L.sfmt = packed ? in_fmt : 0;
    return L;
  };
  a.l1 = layer_of(ys, packed1, s1->in_fmt); a.l2 = layer_of(ys2, packed2, s2->in_fmt);
  // one staged copy of the K2 tables serves both layers when they index the same set the same way (flat.hip's rule for the mix forms)
  if (a.l2.tables == a.l1.tables && a.l2.clamped == a.l1.clamped) a.l2.tables = nullptr;
  a.w = pr->sw; a.h = pr->sh; a.orow = drow;
  a.urow = planar ? sk->orow[1] : 0; a.vrow = planar ? sk->orow[2] : 0;
  if (cv) { a.cw = cv->nwidth; a.ch = cv->nheight; a.ox = cv->offs_x; a.oy = cv->offs_y; }
  a.use_lut = pr->use_lut ? 1 : 0; a.fmt = sk ? sk->out_fmt : 0; a.unclamped = sk ? (sk->which_tables & 1) : 0;
  // the figure, on the frame lgpu_transition / lgpu_dissolve would be run on: 4-byte pixels at the canvas's size
  const TransGeom g = transition_geometry(kind, fw, fh, 4);
  a.kind = kind; a.fw = fw; a.fh = fh; a.wb = g.wb; a.ihwidth = g.ihwidth; a.ihheight = g.ihheight;
  const Lut8 l = pack_lut(pr->use_lut ? pr->lut8 : nullptr);
  const int hw = pr->sw >> 1, nunits = pr->sh / 2 + 1;
  const unsigned gx = cdiv((unsigned)hw, 256u);
  const long long bar_px = cv ? (long long)fw * fh - (long long)pr->sw * pr->sh : 0;
  hipStream_t st = (hipStream_t)stream;
  for (int t0 = 0; t0 < ntracks; t0 += LGPU_CHAIN_SELECT_TRACKS) {
    const int n = std::min(LGPU_CHAIN_SELECT_TRACKS, ntracks - t0);
    // about kFlatWgTarget workgroups per launch, each walking a run of consecutive units on one staging of the tables (flat.hip's launch shape)
    const int cap = std::max(1, (int)(kFlatWgTarget / ((long long)gx * n)));
    int gy = std::min(nunits, cap);
    a.per = (nunits + gy - 1) / gy;
    gy = (nunits + a.per - 1) / a.per;
    a.gy_units = gy;
    const unsigned bar_gy = bar_px > 0 ? (unsigned)std::min<long long>(64, (bar_px + 1024ll * gx - 1) / (1024ll * gx)) : 0u;
    const dim3 grid(gx, (unsigned)gy + bar_gy, (unsigned)n);
    auto fill = [&](auto &T) {
      memset(&T, 0, sizeof T);
      for (int i = 0; i < n; i++) {
        const lgpu_chain_yuv_mix_track &t = tracks[t0 + i];
        T.y[i] = t.y_d; T.u[i] = t.u_d; T.v[i] = t.v_d; T.y2[i] = t.y2_d; T.u2[i] = t.u2_d; T.v2[i] = t.v2_d;
        for (int k = 0; k < nplanes; k++) T.dst[k][i] = t.dst_d[k];
        T.mask[i] = kind == LGPU_SELECT_DISSOLVE ? sel->mask_d[t0 + i] : nullptr;
        T.amt[i] = transition_amount(g, kind, 4, 0, sel->amounts[t0 + i]);
      }
    };
    // THE dispatch point: 3 sinks x SRC x SRC2 x SWAP
#define SEL_LAUNCH_L2(SK, SR, S2) do {                                                                                               \
      SelTracksT<SK == 2 ? 3 : 1> T;                                                                                                 \
      fill(T);                                                                                                                       \
      if (chain_order) hipLaunchKernelGGL((k_flat_select<1, SK, SR, S2>), grid, dim3(256), 0, st, a, T, l);                         \
      else hipLaunchKernelGGL((k_flat_select<0, SK, SR, S2>), grid, dim3(256), 0, st, a, T, l);                                     \
    } while (0)
#define SEL_LAUNCH_SRC(SK, SR) do { if (srcp2 == 2) SEL_LAUNCH_L2(SK, SR, 2); else if (srcp2 == 1) SEL_LAUNCH_L2(SK, SR, 1); else SEL_LAUNCH_L2(SK, SR, 0); } while (0)
#define SEL_LAUNCH(SK) do { if (srcp == 2) SEL_LAUNCH_SRC(SK, 2); else if (srcp == 1) SEL_LAUNCH_SRC(SK, 1); else SEL_LAUNCH_SRC(SK, 0); } while (0)
    if (planar) SEL_LAUNCH(2); else if (sk) SEL_LAUNCH(1); else SEL_LAUNCH(0);
#undef SEL_LAUNCH
#undef SEL_LAUNCH_SRC
#undef SEL_LAUNCH_L2
    LGPU_CHECK_LAUNCH();
  }
  return LGPU_OK;
#undef SEL_REQUIRE
#undef SEL_REFUSE
}
