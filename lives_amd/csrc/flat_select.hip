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
// Table staging and the bar pixels' decode are flat_walk.h's too; the host side -- layer description, track record, refusal sequence, launch shape, dispatch -- is
// flat_plan.h's, behind the select's own checks (kind, amounts, masks).
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
#include "flat_plan.h"      // the host side every unscaled form shares: layer description, track record, refusal sequence, launch shape, dispatch
#include "select_pred.h"
#include <algorithm>
#include <cmath>
#include <string.h>

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
        int x, y;
        flat_bar_xy((int)p, top, bottom, sw_, A.cw, A.ox, A.oy, A.w, A.h, x, y);
        reinterpret_cast<uint32_t *>(T.dst[0][z] + (size_t)y * A.orow)[x] = c;
      }
      return;
    }
  }
  {
    // K2's tables, paired (flat_walk.h).  Layer 2's own copy when its table set or its index clamp differs (a packed layer indexes with the sample itself)
    flat_stage_k2(tid, A.l1.tables, A.l1.clamped, s_ty[0], s_rg[0], s_gb[0]);
    if (A.l2.tables) flat_stage_k2(tid, A.l2.tables, A.l2.clamped, s_ty[1], s_rg[1], s_gb[1]);
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

// k_flat_select's arguments from the plan (flat_plan.h): one function per struct
static SelArgs sel_args(const FlatPlan &p, const FlatLayer &l1, const FlatLayer &l2, int kind, const TransGeom &g) {
  SelArgs a;
  memset(&a, 0, sizeof a);
  flat_fill_layer(a.l1, l1);
  flat_fill_layer(a.l2, l2);
  if (flat_tables_shared(l1, l2)) a.l2.tables = nullptr;
  flat_fill_frame(a, p);
  a.kind = kind; a.fw = p.fw; a.fh = p.fh; a.wb = g.wb; a.ihwidth = g.ihwidth; a.ihheight = g.ihheight;
  return a;
}
template <int NDST> static void sel_fill_tracks(SelTracksT<NDST> &T, const FlatPlan &p, const FlatTrack *tr, const lgpu_select *sel, int t0, int n, const TransGeom &g) {
  memset(&T, 0, sizeof T);
  for (int i = 0; i < n; i++) {
    const FlatTrack &t = tr[t0 + i];
    T.y[i] = t.y; T.u[i] = t.u; T.v[i] = t.v; T.y2[i] = t.y2; T.u2[i] = t.u2; T.v2[i] = t.v2;
    for (int k = 0; k < p.nplanes; k++) T.dst[k][i] = t.dst[k];
    T.mask[i] = sel->kind == LGPU_SELECT_DISSOLVE ? sel->mask_d[t0 + i] : nullptr;
    T.amt[i] = transition_amount(g, sel->kind, 4, 0, sel->amounts[t0 + i]);
  }
}

// lgpu_chain_flat_yuv_select (include/lives_gpu_select.h): the select's own checks -- kind, amounts, masks -- then the refusal sequence of every unscaled form
// (flat_plan): LGPU_E_BADARG before LGPU_E_UNSUPPORTED, everything before anything is allocated or enqueued
extern "C" int lgpu_chain_flat_yuv_select(const lgpu_chain_params *pr, const lgpu_yuv_layer_source *s1, const lgpu_yuv_layer_source *s2, const lgpu_select *sel,
                                          const lgpu_canvas *cv, const lgpu_chain_sink *sk, const lgpu_chain_yuv_mix_track *tracks, int ntracks, void *stream) {
  int rc = ensure_init();
  if (rc) return rc;
  LGPU_REQUIRE(pr && s1 && s2 && sel && tracks && ntracks > 0 && ntracks <= LGPU_CHAIN_MAX_TRACKS, "params, both sources, the select and 1..64 tracks required");
  LGPU_REQUIRE(s1->in_fmt >= 2 && s1->in_fmt <= 5 && s2->in_fmt >= 2 && s2->in_fmt <= 5, "in_fmt must be 2 (UYVY), 3 (YUYV), 4 (YUV420P) or 5 (YUV422P) on either layer");
  LGPU_REQUIRE(!(cv && sk), "a canvas and a sink together: chroma rows would straddle the bar / frame edge");
  const int kind = sel->kind;
  LGPU_REQUIRE(kind == LGPU_SELECT_IRIS_RECT || kind == LGPU_SELECT_IRIS_CIRCLE || kind == LGPU_SELECT_DISSOLVE,
               "kind must be 0 (iris rectangle), 1 (iris circle) or 3 (dissolve); the other transitions show layer 1 at a shifted position or need both layers");
  LGPU_REQUIRE(sel->amounts, "null amounts");
  for (int i = 0; i < ntracks; i++) LGPU_REQUIRE(std::isfinite(sel->amounts[i]) && sel->amounts[i] >= 0. && sel->amounts[i] <= 1., "a transition amount is a finite number in 0..1");
  if (kind == LGPU_SELECT_DISSOLVE) {
    LGPU_REQUIRE(sel->mask_d, "dissolve needs the table of mask pointers");
    for (int i = 0; i < ntracks; i++) {
      LGPU_REQUIRE(sel->mask_d[i], "null dissolve mask");
      LGPU_REQUIRE(multiple_of((uintptr_t)sel->mask_d[i], 4), "a dissolve mask is read as floats (address % 4 == 0)");
    }
  }
  const FlatLayer l1 = flat_layer(s1), l2 = flat_layer(s2);
  FlatTrack tr[LGPU_CHAIN_MAX_TRACKS];
  flat_tracks(tr, tracks, ntracks, l1.packed);
  FlatPlan p;
  if ((rc = flat_plan("lgpu_chain_flat_yuv_select", true, "frames that keep their size only (sw == dw, sh == dh)", pr, l1, &l2, cv, sk, tr, ntracks, nullptr, &p))) return rc;
  // the figure, on the frame lgpu_transition / lgpu_dissolve would be run on: 4-byte pixels at the canvas's size
  const TransGeom g = transition_geometry(kind, p.fw, p.fh, 4);
  SelArgs a = sel_args(p, l1, l2, kind, g);
  hipStream_t st = (hipStream_t)stream;
  for (int t0 = 0; t0 < ntracks; t0 += LGPU_CHAIN_SELECT_TRACKS) {
    const int n = std::min(LGPU_CHAIN_SELECT_TRACKS, ntracks - t0);
    const FlatShape s = flat_launch_shape(p, n);
    a.per = s.per; a.gy_units = s.gy_units;
    // THE dispatch point: 3 sinks x SRC x SRC2 x SWAP
    with_constant<3>(p.sink, [&](auto sink) { with_constant<3>(l1.policy, [&](auto src) { with_constant<3>(l2.policy, [&](auto src2) { with_constant<2>(p.chain_order, [&](auto swap) {
      constexpr int SK = decltype(sink)::value;
      SelTracksT<SK == 2 ? 3 : 1> T;
      sel_fill_tracks(T, p, tr, sel, t0, n, g);
      hipLaunchKernelGGL((k_flat_select<decltype(swap)::value, SK, decltype(src)::value, decltype(src2)::value>), s.grid, dim3(256), 0, st, a, T, p.lut);
    }); }); }); });
    LGPU_CHECK_LAUNCH();
  }
  return LGPU_OK;
}
