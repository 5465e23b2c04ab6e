// flat.hip -- the UNSCALED tick from decoded planar YUV 4:2:0 frames in one launch (lgpu_chain_flat_yuv420p, lgpu_chain_flat_yuv420p_to_yuv):
// K2's conversion (yuv.hip, every quirk kept) -> [R <-> B] [-> letterbox onto opaque black] [-> chroma blend with layer 2] [-> gamma LUT] -> RGBA, or -> K4's
// conversion (palette.hip, every quirk kept) to UYVY / YUYV / YUV420P.  No RGBA frame is read or written in between: 1.5 + 4 + 4 bytes per pixel to RGBA with a
// blend instead of 17.5 over two launches, 1.5 + 4 + 1.5 to YUV420P instead of 23 over three.
//
// No scaler, no LDS window, no cross-lane exchange.  A lane owns one (unit, chroma column k) cell of K2's walk -- unit 0 = row 0, unit p >= 1 = rows (2p - 1, 2p),
// then (even heights) the trailing row -- that is two pixels of one row or a 2 x 2 quad.  K4's 4:2:0 chroma walk pairs the rows the same way: chroma row r is
// cavg(row 2r + 2, row 2r + 1) with U of a pair's first pixel and V of its second, and the last chroma row is row dh - 1's alone (palette.hip, k_rgb_to_yuv FMT 4).
// So unit p feeds chroma row p - 1 from the quad it already holds, unit 0 gives luma only, and the trailing-row unit of an even height gives the last chroma row.
// Which chroma sample feeds which pixel is k2_walk.h's word, here as in yuv.hip and pixbuf.hip (sites that keep their own text name the header's function they repeat).
//
// Tables: K2's as in k_yuv420p_to_rgb_s (RGB_Y, {R_Cr, G_Cr}[v], {G_Cb, B_Cb}[u] with the chroma clamp folded into the index: 5 KB), the LUT (256 B) and, with a
// sink, the {Y, U} / {Y, V} tables of get_sink_tables (12 KB), all staged in LDS once per workgroup; a workgroup then walks a run of consecutive units.
//
// lgpu_chain_flat_yuv420p_mix (the L2YUV policy): layer 2 is a decoded 4:2:0 frame of the same size.  The lane that owns a cell of layer 1 owns the same cell of layer
// 2 and converts it with the same walk (flat_cell) under layer 2's own description; 1.5 + 1.5 + 4 bytes per pixel to RGBA and no RGBA frame anywhere.
//
// lgpu_chain_flat_yuv422 (the SRC policy): layer 1 is a planar 4:2:2 frame (YUV422P) or a packed one (UYVY / YUYV).  The unit walk, emit and the sink stores stay; a lane
// converts its two pixels of each row of its unit with flat_row422 -- yuv.hip's 4:2:2 walk with the reference's seed quirk, or K3's macropixel conversion.
//
// lgpu_chain_flat_yuv_mix: L2YUV is layer 2's source policy as SRC is layer 1's (1 planar 4:2:0, 2 YUV422P, 3 packed), and the two combine freely: a camera fading
// into a decoded clip, two 4:2:2 clips in a transition, a 4:2:0 clip into a 4:2:2 one -- each one launch with no RGBA frame anywhere.
//
// Host side: every entry point describes its layers (flat_layer) and tracks (FlatTrack) and calls flat_run: the refusal sequence and the plan (flat_plan), FlatArgs
// and the tracks struct filled from them, the launch shape, one dispatch point.  flat_plan.h declares what flat_select.hip's entry point shares; it is defined here.
#include "lgpu_common.h"
#include "k2_walk.h"
#include "flat_walk.h"      // flat_cell, flat_row422, flat_cell422, flat_stage_k2, flat_bar_xy: the device text shared with flat_select.hip
#include "flat_plan.h"      // the host side shared with flat_select.hip (defined below): layer description, track record, refusal sequence, launch shape, dispatch
#include <algorithm>
#include <string.h>

namespace lgpu { int cavg_forms_checked(); }      // palette.hip
int get_sink_tables(int which_tables, int in_order, const uint2 **out);      // pixbuf.hip

namespace lgpu {

constexpr int kFlatPlanarTracks = 32;     // tracks per launch with the 4:2:0 sink (seven pointers per track: 64 would not fit HIP's 4 KB of kernel arguments)

struct FlatArgs {
  const int32_t *tables;         // device [5][256] RGB_Y R_Cr G_Cb G_Cr B_Cb
  const uint2 *stab;             // sink: device [2][3][256] (get_sink_tables)
  uint32_t usize, vsize;         // chroma plane bytes; K2's read one past the last row's end is clamped to the last byte
  int ys, us, vs;
  int w, h;                      // the frame
  int orow, irow2;               // destination (RGBA / packed / luma) and layer-2 rowstrides
  int urow, vrow;                // 4:2:0 sink: chroma rowstrides
  int cw, ch, ox, oy;            // canvas (cw == 0: none)
  int clamped, lowq, fix_edges, use_lut;
  int fmt, unclamped;            // sink: 2 UYVY, 3 YUYV, 4 YUV420P
  int gy_units, per;             // blockIdx.y < gy_units: the workgroup walks units [y * per, (y + 1) * per); the others write the canvas's bars
  int sfmt;                      // SRC == 2: 2 UYVY, 3 YUYV (wave-uniform, as fmt is for the sink).  It sits in what was the struct's tail padding: no other offset moves
};
static_assert(sizeof(FlatArgs) == 112, "the argument layout of the SRC == 0 instantiations is fixed (docs/KERNELS.md, k_flat_yuv420<.., SRC>)");
template <int NT, int NDST> struct FlatTracksT {
  const uint8_t *y[NT], *u[NT], *v[NT], *l2[NT];
  uint8_t *dst[NDST][NT];
  uint8_t bf[NT];
};
// L2YUV: layer 2 is a decoded frame too (lgpu_chain_flat_yuv420p_mix, lgpu_chain_flat_yuv_mix).  Its description travels with the tracks, so FlatArgs and the argument
// layout of the L2YUV = 0 instantiations stay what they were
template <int NT, int NDST> struct FlatMixTracksT {
  const uint8_t *y[NT], *u[NT], *v[NT], *y2[NT], *u2[NT], *v2[NT];
  uint8_t *dst[NDST][NT];
  uint8_t bf[NT];
  const int32_t *tables2;        // layer 2's device [5][256]; null: src2 names layer 1's tables and the one staged copy serves both
  uint32_t usize2, vsize2;
  int ys2, us2, vs2;
  int clamped2, lowq2, fix_edges2;
};
// L2YUV == 3: layer 2's packed format rides at the tail, so no offset of the planar forms moves (theirs is the struct above, as it was)
template <int NT, int NDST> struct FlatMixTracksPackedT : FlatMixTracksT<NT, NDST> {
  int sfmt2;                     // 2 UYVY, 3 YUYV (wave-uniform, as FlatArgs::sfmt is for layer 1)
};
// L2YUV, layer 2's source policy: 0 an RGBA frame or none, 1 planar 4:2:0, 2 planar 4:2:2 (YUV422P), 3 packed 4:2:2 (UYVY / YUYV)
template <int SINK, int L2YUV = 0> struct FlatTr { typedef FlatMixTracksT<LGPU_CHAIN_MIX_TRACKS, SINK == 2 ? 3 : 1> type; };
template <int SINK> struct FlatTr<SINK, 0> { typedef FlatTracksT<LGPU_CHAIN_MAX_TRACKS, 1> type; };
template <> struct FlatTr<2, 0> { typedef FlatTracksT<kFlatPlanarTracks, 3> type; };
template <int SINK> struct FlatTr<SINK, 3> { typedef FlatMixTracksPackedT<LGPU_CHAIN_MIX_TRACKS, SINK == 2 ? 3 : 1> type; };
template <int SINK> struct FlatSinkLds { uint2 t[6 * 256]; };
template <> struct FlatSinkLds<0> {};
template <int L2YUV> struct FlatL2Lds { uint32_t ty[256]; uint2 rg[256], gb[256]; };      // layer 2's own K2 tables (5 KB), staged when its table set or index clamp differs
template <> struct FlatL2Lds<0> {};
static_assert(sizeof(FlatArgs) + sizeof(FlatTr<0>::type) + sizeof(Lut8) <= 4096 && sizeof(FlatArgs) + sizeof(FlatTr<2>::type) + sizeof(Lut8) <= 4096 &&
              sizeof(FlatArgs) + sizeof(FlatTr<0, 1>::type) + sizeof(Lut8) <= 4096 && sizeof(FlatArgs) + sizeof(FlatTr<2, 1>::type) + sizeof(Lut8) <= 4096 &&
              sizeof(FlatArgs) + sizeof(FlatTr<0, 2>::type) + sizeof(Lut8) <= 4096 && sizeof(FlatArgs) + sizeof(FlatTr<2, 2>::type) + sizeof(Lut8) <= 4096 &&
              sizeof(FlatArgs) + sizeof(FlatTr<0, 3>::type) + sizeof(Lut8) <= 4096 && sizeof(FlatArgs) + sizeof(FlatTr<2, 3>::type) + sizeof(Lut8) <= 4096,
              "HIP documents 4 KB of arguments for a __global__ function");

// SINK: 0 RGBA, 1 packed 4:2:2 (UYVY / YUYV), 2 planar 4:2:0.  SWAP: the finished pixel is BGRA (src->out_order ^ params->swap_rb).  L2YUV: layer 2 is a decoded frame
// of the same size (BLEND is 1; with a canvas, lgpu_chain_flat_yuv_mix_canvas, both layers sit at the same place on it) -- 1 planar 4:2:0, 2 planar 4:2:2, 3 packed 4:2:2 (T.sfmt2: UYVY / YUYV; T.y2 is the frame, T.u2 / T.v2 are not read): the
// lane converts ITS cell of layer 2 first, with that format's walk, keeps the two or four finished pixels and only then walks layer 1, so the temporaries of the
// two walks are never live together.  Layer 2's alpha is 255 by construction: the blend is the opaque one.  L2YUV and SRC combine freely.
// SRC: layer 1 is 0 planar 4:2:0, 1 planar 4:2:2 (YUV422P), 2 packed 4:2:2 (A.sfmt: UYVY / YUYV; T.y is the frame, T.u / T.v are not read).  The units, emit and
// the chroma-row stores are the same for all three: a 4:2:2 lane owns two pixels of each row of its unit too (flat_cell422)
template <int BLEND, int SWAP, int SINK, int L2YUV = 0, int SRC = 0>
__global__ __launch_bounds__(256) void k_flat_yuv420(const FlatArgs A, const typename FlatTr<SINK, L2YUV>::type T, const Lut8 lut) {
  static_assert(SRC >= 0 && SRC <= 2 && L2YUV >= 0 && L2YUV <= 3, "SRC: 0 4:2:0, 1 YUV422P, 2 packed; L2YUV: 0 RGBA or none, then the same three as SRC + 1");
  __shared__ uint32_t s_ty[256];
  __shared__ uint2 s_rg[256], s_gb[256];
  __shared__ __attribute__((aligned(16))) uint8_t s_lut[256];
  __shared__ FlatSinkLds<SINK> s_sink;
  __shared__ FlatL2Lds<L2YUV> s_l2;
  const int tid = threadIdx.x, z = blockIdx.z;
  const uint32_t bf = BLEND ? (uint32_t)T.bf[z] : 0u, nbf = 255u - bf;
  stage_lut(s_lut, lut);
  if constexpr (SINK == 0) {
    if ((int)blockIdx.y >= A.gy_units) {
      // letterbox bars (letterbox_layer's black canvas under the rest of the chain): opaque black [-> chroma blend with layer 2] [-> LUT].  L2YUV: layer 2 is
      // letterboxed onto the same canvas, so its bar pixel is opaque black too and nothing is read
      __syncthreads();
      const int bb = ((int)blockIdx.y - A.gy_units) * (int)gridDim.x + (int)blockIdx.x, nbb = ((int)gridDim.y - A.gy_units) * (int)gridDim.x;
      const int top = A.oy * A.cw, bottom = (A.ch - A.oy - A.h) * A.cw, sw_ = A.cw - A.w, total = top + bottom + A.h * sw_;
      for (long p = (long)bb * 256 + tid; p < total; p += (long)nbb * 256) {
        int x, y;
        flat_bar_xy((int)p, top, bottom, sw_, A.cw, A.ox, A.oy, A.w, A.h, x, y);
        uint32_t c = 0xFF000000u;
        if constexpr (L2YUV) c = pb_chroma_opaque(c, 0xFF000000u, bf, nbf);
        else if (BLEND) c = pb_chroma_rgba(c, reinterpret_cast<const uint32_t *>(T.l2[z] + (size_t)y * A.irow2)[x], bf, nbf);
        if (A.use_lut) c = lut3_rgba(s_lut, c);
        reinterpret_cast<uint32_t *>(T.dst[0][z] + (size_t)y * A.orow)[x] = c;
      }
      return;
    }
  }
  {
    flat_stage_k2(tid, A.tables, A.clamped, s_ty, s_rg, s_gb);
    if constexpr (SINK != 0) {
#pragma unroll
      for (int i = 0; i < 6; i++) s_sink.t[tid + 256 * i] = A.stab[tid + 256 * i];
    }
    if constexpr (L2YUV) {
      if (T.tables2) flat_stage_k2(tid, T.tables2, T.clamped2, s_l2.ty, s_l2.rg, s_l2.gb);        // layer 2's own tables, its own chroma clamp in the index
    }
  }
  __syncthreads();
  const int hw = A.w >> 1, H = A.h;
  const int k = (int)blockIdx.x * 256 + tid;
  if (k >= hw) return;
  const int npairs = (H - 1) / 2;                            // full row pairs starting at row 1
  const int nunits = 1 + npairs + (((H - 1) & 1) ? 1 : 0);
  const FlatPlanes P1 = {T.y[z], T.u[z], T.v[z], A.usize, A.vsize, A.ys, A.us, A.vs, A.lowq, A.fix_edges};
  const FlatK2Lds L1 = {s_ty, s_rg, s_gb};
  // the rest of the chain on the two pixels of frame row i, then the store; q0 / q1: layer 2's two pixels (L2YUV; read from the RGBA frame otherwise); cu / cv: the
  // clamped U of the first pixel and V of the second (4:2:0 sink)
  auto emit = [&](int i, uint32_t p0, uint32_t p1, uint32_t q0, uint32_t q1, int &cu, int &cv) __attribute__((always_inline)) {
    if constexpr (L2YUV) {
      p0 = pb_chroma_opaque(p0, q0, bf, nbf); p1 = pb_chroma_opaque(p1, q1, bf, nbf);
    } else if (BLEND) {
      const uint8_t *l = T.l2[z] + (size_t)(i + A.oy) * A.irow2 + 4 * (size_t)(2 * k + A.ox);
      if (multiple_of(reinterpret_cast<uintptr_t>(l), 8)) { const uint2 q = *reinterpret_cast<const uint2 *>(l); q0 = q.x; q1 = q.y; }
      else { q0 = reinterpret_cast<const uint32_t *>(l)[0]; q1 = reinterpret_cast<const uint32_t *>(l)[1]; }
      p0 = pb_chroma_rgba(p0, q0, bf, nbf); p1 = pb_chroma_rgba(p1, q1, bf, nbf);
    }
    if (A.use_lut) { p0 = lut3_rgba(s_lut, p0); p1 = lut3_rgba(s_lut, p1); }
    if constexpr (SINK == 0) {
      uint8_t *d = T.dst[0][z] + (size_t)(i + A.oy) * A.orow + 4 * (size_t)(2 * k + A.ox);
      if (multiple_of(reinterpret_cast<uintptr_t>(d), 8)) *reinterpret_cast<uint2 *>(d) = make_uint2(p0, p1);
      else { reinterpret_cast<uint32_t *>(d)[0] = p0; reinterpret_cast<uint32_t *>(d)[1] = p1; }
    } else {
      // K4 (k_pb_half's sink_row): the nine table sums >> 16 as a short, upper clamp then lower
      const uint2 *tu = s_sink.t, *tv = s_sink.t + 768;
      const uint2 a0 = tu[p0 & 0xFF], b0 = tu[256 + ((p0 >> 8) & 0xFF)], c0 = tu[512 + ((p0 >> 16) & 0xFF)];
      const uint2 a1 = tv[p1 & 0xFF], b1 = tv[256 + ((p1 >> 8) & 0xFF)], c1 = tv[512 + ((p1 >> 16) & 0xFF)];
      const int min_y = A.unclamped ? 0 : 16, max_y = A.unclamped ? 255 : 235, min_uv = min_y, max_uv = A.unclamped ? 255 : 240;
      const int ya = (int)(a0.x + b0.x + c0.x) >> 16, yb = (int)(a1.x + b1.x + c1.x) >> 16;
      const int ur = (int)(a0.y + b0.y + c0.y) >> 16, vr = (int)(a1.y + b1.y + c1.y) >> 16;
      const uint32_t y0c = (uint32_t)min(max(ya, min_y), max_y), y1c = (uint32_t)min(max(yb, min_y), max_y);
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
    int cu0 = 0, cv0 = 0, cu1 = 0, cv1 = 0;
    uint32_t q[4] = {0u, 0u, 0u, 0u};
    if constexpr (L2YUV) {
      const FlatPlanes P2 = {T.y2[z], T.u2[z], T.v2[z], T.usize2, T.vsize2, T.ys2, T.us2, T.vs2, T.lowq2, T.fix_edges2};
      const bool own = T.tables2 != nullptr;      // wave-uniform
      const FlatK2Lds L2 = {own ? s_l2.ty : s_ty, own ? s_l2.rg : s_rg, own ? s_l2.gb : s_gb};
      auto keep = [&](auto, int, int, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) __attribute__((always_inline)) {
        q[0] = a0; q[1] = a1; q[2] = b0; q[3] = b1;
      };
      if constexpr (L2YUV == 1) flat_cell<SWAP>(P2, L2, unit, k, hw, H, npairs, keep);
      else if constexpr (L2YUV == 2) flat_cell422<SWAP, 1>(P2, L2, 0, unit, k, H, npairs, keep);
      else flat_cell422<SWAP, 2>(P2, L2, T.sfmt2, unit, k, H, npairs, keep);
    }
    auto rows = [&](auto cell, int i, int r, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) __attribute__((always_inline)) {
      constexpr int kind = decltype(cell)::value;
      emit(i, a0, a1, q[0], q[1], cu0, cv0);       // row 0's chroma is never kept
      if constexpr (kind == 1) {
        emit(i + 1, b0, b1, q[2], q[3], cu1, cv1);
        if constexpr (SINK == 2) {      // chroma row r = cavg(row 2r + 2, row 2r + 1): the argument order of the reference
          const int cl = !A.unclamped;
          T.dst[1][z][(size_t)r * A.urow + k] = (uint8_t)cavg_arith(cl, cu1, cu0);
          T.dst[2][z][(size_t)r * A.vrow + k] = (uint8_t)cavg_arith(cl, cv1, cv0);
        }
      }
      if constexpr (kind == 2 && SINK == 2) {      // the last chroma row is row dh - 1's alone
        T.dst[1][z][(size_t)r * A.urow + k] = (uint8_t)cu0;
        T.dst[2][z][(size_t)r * A.vrow + k] = (uint8_t)cv0;
      }
    };
    if constexpr (SRC == 0) flat_cell<SWAP>(P1, L1, unit, k, hw, H, npairs, rows);
    else flat_cell422<SWAP, SRC>(P1, L1, A.sfmt, unit, k, H, npairs, rows);
  }
}

}  // namespace lgpu

using namespace lgpu;

// ---- the plan of every lgpu_chain_flat_* entry point (flat_plan.h) ----
static FlatLayer make_layer(int fmt, const int istrides[3], long u_size, long v_size, int out_order, int which_tables, int pb_quality, int flags) {
  FlatLayer l;
  memset(&l, 0, sizeof l);
  l.fmt = fmt; l.packed = fmt == 2 || fmt == 3; l.policy = l.packed ? 2 : fmt == 5 ? 1 : 0;
  l.ys.istrides[0] = istrides[0];
  if (!l.packed) { l.ys.istrides[1] = istrides[1]; l.ys.istrides[2] = istrides[2]; l.ys.u_size = u_size; l.ys.v_size = v_size; }
  l.ys.out_order = out_order; l.ys.which_tables = which_tables; l.ys.pb_quality = pb_quality; l.ys.flags = flags;
  l.tables = device_tables()->yuv2rgb[which_tables & 3];
  l.clamped = !l.packed && !(which_tables & 1);
  l.lowq = pb_quality == 1; l.fix_edges = (flags & LGPU_YUV_FIX_EDGES) ? 1 : 0; l.sfmt = l.packed ? fmt : 0;
  return l;
}
FlatLayer lgpu::flat_layer(const lgpu_yuv_source *s) { return make_layer(4, s->istrides, s->u_size, s->v_size, s->out_order, s->which_tables, s->pb_quality, s->flags); }
FlatLayer lgpu::flat_layer(const lgpu_yuv422_source *s) { return make_layer(s->in_fmt, s->istrides, s->u_size, s->v_size, s->out_order, s->which_tables, s->pb_quality, 0); }
FlatLayer lgpu::flat_layer(const lgpu_yuv_layer_source *s) {
  return make_layer(s->in_fmt, s->istrides, s->u_size, s->v_size, s->out_order, s->which_tables, s->pb_quality, s->flags);
}

void lgpu::flat_tracks(FlatTrack *out, const lgpu_chain_yuv_mix_track *tracks, int ntracks, bool packed1) {
  for (int i = 0; i < ntracks; i++) {
    const lgpu_chain_yuv_mix_track &t = tracks[i];
    out[i] = {t.y_d, packed1 ? nullptr : t.u_d, packed1 ? nullptr : t.v_d, nullptr, t.y2_d, t.u2_d, t.v2_d, {t.dst_d[0], t.dst_d[1], t.dst_d[2]}};
  }
}
// from the sink forms' tracks (a packed layer 1's chroma pointers stay the caller's: a destination must not be one of them)
static void flat_sink_tracks(FlatTrack *out, const lgpu_chain_yuv_sink_track *tracks, int ntracks) {
  for (int i = 0; i < ntracks; i++) {
    const lgpu_chain_yuv_sink_track &t = tracks[i];
    out[i] = {t.y_d, t.u_d, t.v_d, t.layer2_d, nullptr, nullptr, nullptr, {t.dst_d[0], t.dst_d[1], t.dst_d[2]}};
  }
}

#define FLAT_REQUIRE(cond, msg) do { if (!(cond)) { set_error("%s: %s", fn, msg); return LGPU_E_BADARG; } } while (0)
#define FLAT_REFUSE(msg) do { set_error("%s: %s", fn, msg); return LGPU_E_UNSUPPORTED; } while (0)
int lgpu::flat_plan(const char *fn, bool select, const char *keep_size, const lgpu_chain_params *pr, const FlatLayer &l1, const FlatLayer *l2, const lgpu_canvas *cv,
                    const lgpu_chain_sink *sk, const FlatTrack *tracks, int ntracks, const uint8_t *amounts, FlatPlan *plan) {
  FlatPlan &p = *plan;
  memset(&p, 0, sizeof p);
  p.noblend = !select && (pr->interp & LGPU_INTERP_NOBLEND) != 0;
  p.l2rgba = !select && !p.noblend && !l2;
  FLAT_REQUIRE(pr->interp & LGPU_INTERP_PIXBUF, "the gdk-pixbuf arithmetic only (LGPU_INTERP_PIXBUF)");
  if (!select) {
    FLAT_REQUIRE(!l2 || !p.noblend, "LGPU_INTERP_NOBLEND leaves nothing to mix: lgpu_chain_flat_yuv420p[_to_yuv]");
    FLAT_REQUIRE(amounts || p.noblend, "null amounts");
  }
  int rc;
  if ((rc = check_yuv_source(fn, pr, &l1.ys, l1.fmt)) || (l2 && (rc = check_yuv_source(fn, pr, &l2->ys, l2->fmt)))) return rc;
  p.chain_order = (l1.ys.out_order ^ (pr->swap_rb ? 1 : 0)) & 1;
  FLAT_REQUIRE(!l2 || l2->ys.out_order == p.chain_order,
               select ? "src2->out_order must state the byte order the select works in: src->out_order ^ params->swap_rb"
                      : "src2->out_order must state the byte order the blend works in: src->out_order ^ params->swap_rb");
  p.planar = sk && sk->out_fmt >= 4;
  p.nplanes = p.planar ? 3 : 1; p.sink = p.planar ? 2 : sk ? 1 : 0;
  p.fw = cv && !sk ? cv->nwidth : pr->dw; p.fh = cv && !sk ? cv->nheight : pr->dh;
  if ((rc = sk ? check_yuv_sink(fn, pr, sk, p.chain_order, p.l2rgba) : check_rgba_dest(fn, pr, cv, p.l2rgba))) return rc;
  const bool packed2 = l2 && l2->packed;
  uintptr_t pb = 0, sb = 0, sb2 = 0;
  for (int i = 0; i < ntracks; i++) {
    const FlatTrack &t = tracks[i];
    const uint8_t *const planes[3] = {t.y, t.u, t.v};
    if ((rc = check_track(fn, planes, l1.packed ? 1 : 3, false, t.l2, p.l2rgba, t.dst, p.nplanes, !sk))) return rc;
    if (l2) {
      // a packed layer 2 is y2 alone: its chroma pointers are not read, so they may be null and are no plane a destination could collide with
      const uint8_t *const u2 = packed2 ? nullptr : t.u2, *const v2 = packed2 ? nullptr : t.v2;
      FLAT_REQUIRE(t.y2 && (packed2 || (u2 && v2)), "null layer-2 plane");
      for (int k = 0; k < p.nplanes; k++)
        FLAT_REQUIRE((const uint8_t *)t.dst[k] != t.y2 && (const uint8_t *)t.dst[k] != u2 && (const uint8_t *)t.dst[k] != v2, "a destination plane is one of layer 2's planes");
      sb2 |= (uintptr_t)t.y2;
    }
    sb |= (uintptr_t)t.y; pb |= (uintptr_t)t.dst[0];
  }
  // the one-launch form; anything else is refused, never run some other way
  if (pr->sw != pr->dw || pr->sh != pr->dh) FLAT_REFUSE(keep_size);
  if (pr->do_blur) FLAT_REFUSE("the gaussian is not offered with a 4:2:0 or 4:2:2 source");
  // K3 reads a macropixel as one aligned dword; the reference divides that rowstride by 4 (docs/QUIRKS.md, K3-c): there is no behaviour to follow elsewhere
  if (l1.packed && !multiple_of(sb | (uintptr_t)l1.ys.istrides[0], 4)) FLAT_REFUSE("a UYVY / YUYV source is read as 4-byte macropixels (plane and rowstride % 4 == 0)");
  if (packed2 && !multiple_of(sb2 | (uintptr_t)l2->ys.istrides[0], 4)) FLAT_REFUSE("a UYVY / YUYV layer 2 is read as 4-byte macropixels (plane and rowstride % 4 == 0)");
  if (sk) {
    if (sk->out_fmt == 5)
      FLAT_REFUSE(select ? "YUV422P is not served (the RGBA form + lgpu_rgb_to_yuv_batch)" : "YUV422P is not served (lgpu_chain_flat_yuv420p + lgpu_rgb_to_yuv_batch)");
    if (p.planar && (pr->dh & 1)) FLAT_REFUSE("the 4:2:0 sink needs an even height");
    // a lane stores one macropixel (4 bytes) or one luma pair (2 bytes) per row; chroma samples are single bytes
    if (!multiple_of(pb | (uintptr_t)sk->orow[0], p.planar ? 2 : 4))
      FLAT_REFUSE("packed sinks are stored as 4-byte macropixels (plane and rowstride % 4 == 0), the 4:2:0 luma plane as 2-byte pairs (plane and rowstride % 2 == 0)");
  }
  p.drow = sk ? sk->orow[0] : pr->orow; p.irow2 = p.l2rgba ? pr->irow2 : 0;
  p.urow = p.planar ? sk->orow[1] : 0; p.vrow = p.planar ? sk->orow[2] : 0;
  if ((rc = check_plane_sizes(fn, {(long long)pr->sh * l1.ys.istrides[0], l1.ys.u_size, l1.ys.v_size, (long long)p.fh * p.drow, (long long)p.fh * p.irow2,
                                   l2 ? (long long)pr->sh * l2->ys.istrides[0] : 0, l2 ? l2->ys.u_size : 0, l2 ? l2->ys.v_size : 0,
                                   (long long)(pr->dh >> 1) * p.urow, (long long)(pr->dh >> 1) * p.vrow}))) return rc;
  if (p.planar && (rc = cavg_forms_checked())) return rc;
  if (sk && (rc = get_sink_tables(sk->which_tables, sk->in_order, &p.stab))) return rc;
  p.w = pr->sw; p.h = pr->sh;
  if (cv) { p.cw = cv->nwidth; p.ch = cv->nheight; p.ox = cv->offs_x; p.oy = cv->offs_y; }
  p.fmt = sk ? sk->out_fmt : 0; p.unclamped = sk ? (sk->which_tables & 1) : 0; p.use_lut = pr->use_lut ? 1 : 0;
  p.lut = pack_lut(pr->use_lut ? pr->lut8 : nullptr);
  p.hw = pr->sw >> 1; p.nunits = pr->sh / 2 + 1;
  p.gx = cdiv((unsigned)p.hw, 256u);
  p.bar_px = cv ? (long long)p.fw * p.fh - (long long)pr->sw * pr->sh : 0;
  return LGPU_OK;
}
#undef FLAT_REQUIRE
#undef FLAT_REFUSE

FlatShape lgpu::flat_launch_shape(const FlatPlan &p, int n) {
  FlatShape s;
  const int cap = std::max(1, (int)(kFlatWgTarget / ((long long)p.gx * n)));
  int gy = std::min(p.nunits, cap);
  s.per = (p.nunits + gy - 1) / gy;
  s.gy_units = (p.nunits + s.per - 1) / s.per;
  const unsigned bar_gy = p.bar_px > 0 ? (unsigned)std::min<long long>(64, (p.bar_px + 1024ll * p.gx - 1) / (1024ll * p.gx)) : 0u;
  s.grid = dim3(p.gx, (unsigned)s.gy_units + bar_gy, (unsigned)n);
  return s;
}

// ---- k_flat_yuv420's arguments from the plan: one function per struct ----
static FlatArgs flat_args(const FlatPlan &p, const FlatLayer &l1) {
  FlatArgs a;
  memset(&a, 0, sizeof a);
  flat_fill_layer(a, l1);
  flat_fill_frame(a, p);
  a.irow2 = p.irow2;
  return a;
}
template <int NT, int NDST>
static void flat_fill_tracks(FlatTracksT<NT, NDST> &T, const FlatPlan &p, const FlatLayer &, const FlatLayer *, const FlatTrack *tr, const uint8_t *amounts, int n) {
  for (int i = 0; i < n; i++) {
    T.y[i] = tr[i].y; T.u[i] = tr[i].u; T.v[i] = tr[i].v; T.l2[i] = p.noblend ? nullptr : tr[i].l2; T.bf[i] = amounts ? amounts[i] : 0;
    for (int k = 0; k < p.nplanes; k++) T.dst[k][i] = tr[i].dst[k];
  }
}
template <int NT, int NDST>
static void flat_fill_tracks(FlatMixTracksT<NT, NDST> &T, const FlatPlan &p, const FlatLayer &l1, const FlatLayer *l2, const FlatTrack *tr, const uint8_t *amounts, int n) {
  for (int i = 0; i < n; i++) {
    T.y[i] = tr[i].y; T.u[i] = tr[i].u; T.v[i] = tr[i].v; T.y2[i] = tr[i].y2; T.u2[i] = tr[i].u2; T.v2[i] = tr[i].v2; T.bf[i] = amounts[i];
    for (int k = 0; k < p.nplanes; k++) T.dst[k][i] = tr[i].dst[k];
  }
  T.tables2 = flat_tables_shared(l1, *l2) ? nullptr : l2->tables;
  T.usize2 = (uint32_t)l2->ys.u_size; T.vsize2 = (uint32_t)l2->ys.v_size; T.ys2 = l2->ys.istrides[0]; T.us2 = l2->ys.istrides[1]; T.vs2 = l2->ys.istrides[2];
  T.clamped2 = l2->clamped; T.lowq2 = l2->lowq; T.fix_edges2 = l2->fix_edges;
}
template <int NT, int NDST>
static void flat_fill_tracks(FlatMixTracksPackedT<NT, NDST> &T, const FlatPlan &p, const FlatLayer &l1, const FlatLayer *l2, const FlatTrack *tr, const uint8_t *amounts, int n) {
  flat_fill_tracks(static_cast<FlatMixTracksT<NT, NDST> &>(T), p, l1, l2, tr, amounts, n);
  T.sfmt2 = l2->sfmt;
}

// the six entry points of this file behind their own null checks: the plan, then one launch per 64 tracks (32 with a decoded layer 2 or the 4:2:0 sink).  l2: the mix forms'
// decoded layer 2 (both layers are letterboxed onto cv then), null otherwise
static int flat_run(const char *fn, const lgpu_chain_params *pr, const FlatLayer &l1, const FlatLayer *l2, const lgpu_canvas *cv, const lgpu_chain_sink *sk,
                    const FlatTrack *tr, int ntracks, const uint8_t *amounts, void *stream) {
  FlatPlan p;
  const int rc = flat_plan(fn, false,
                           l1.policy ? "frames that keep their size only (sw == dw, sh == dh); convert with lgpu_yuv420p_to_rgb_batch (is_422) / lgpu_yuv_to_rgb_batch and run lgpu_chain_amounts"
                           : sk ? "frames that keep their size only (sw == dw, sh == dh); the exact 2:1 reduction is lgpu_chain_yuv420p_to_yuv"
                                : "frames that keep their size only (sw == dw, sh == dh); the exact 2:1 reduction is lgpu_chain_yuv420p",
                           pr, l1, l2, cv, sk, tr, ntracks, amounts, &p);
  if (rc) return rc;
  FlatArgs a = flat_args(p, l1);
  const int per_launch = l2 ? LGPU_CHAIN_MIX_TRACKS : p.planar ? kFlatPlanarTracks : LGPU_CHAIN_MAX_TRACKS;
  const int blend = l2 ? 2 + l2->policy : p.noblend ? 0 : 1;      // 0 none, 1 with an RGBA layer 2, 2.. with a decoded one: L2YUV + 1
  hipStream_t st = (hipStream_t)stream;
  for (int t0 = 0; t0 < ntracks; t0 += per_launch) {
    const int n = std::min(per_launch, ntracks - t0);
    const FlatShape s = flat_launch_shape(p, n);
    a.per = s.per; a.gy_units = s.gy_units;
    // THE dispatch point: 3 sinks x SRC x {no blend, RGBA layer 2, L2YUV 1..3} x SWAP, the six of lgpu_chain_flat_yuv420p_mix (SRC 0, L2YUV 1) among them
    with_constant<3>(p.sink, [&](auto sink) { with_constant<3>(l1.policy, [&](auto src) { with_constant<5>(blend, [&](auto bl) { with_constant<2>(p.chain_order, [&](auto swap) {
      constexpr int SK = decltype(sink)::value, SR = decltype(src)::value, BL = decltype(bl)::value, L2 = BL > 1 ? BL - 1 : 0, SW = decltype(swap)::value;
      typename FlatTr<SK, L2>::type T;
      memset(&T, 0, sizeof T);
      flat_fill_tracks(T, p, l1, l2, tr + t0, amounts ? amounts + t0 : nullptr, n);
      hipLaunchKernelGGL((k_flat_yuv420<(BL > 0 ? 1 : 0), SW, SK, L2, SR>), s.grid, dim3(256), 0, st, a, T, p.lut);
    }); }); }); });
    LGPU_CHECK_LAUNCH();
  }
  return LGPU_OK;
}

// lgpu_chain_flat_yuv420p: lgpu_yuv420p_to_rgb (opsize 4, src->out_order, no LUT) + lgpu_chain_amounts with sw == dw, sh == dh, as ONE launch (the canvas's bars
// included); every argument is checked before anything is enqueued
extern "C" int lgpu_chain_flat_yuv420p(const lgpu_chain_params *pr, const lgpu_yuv_source *ys, const lgpu_canvas *cv, const lgpu_chain_yuv_track *tracks, int ntracks,
                                       const uint8_t *amounts, void *stream) {
  int rc = ensure_init();
  if (rc) return rc;
  LGPU_REQUIRE(pr && ys && tracks && ntracks > 0 && ntracks <= LGPU_CHAIN_MAX_TRACKS, "params, source and 1..64 tracks required");
  FlatTrack tr[LGPU_CHAIN_MAX_TRACKS];
  for (int i = 0; i < ntracks; i++) tr[i] = {tracks[i].y_d, tracks[i].u_d, tracks[i].v_d, tracks[i].layer2_d, nullptr, nullptr, nullptr, {tracks[i].dst_d, nullptr, nullptr}};
  return flat_run("lgpu_chain_flat_yuv420p", pr, flat_layer(ys), nullptr, cv, nullptr, tr, ntracks, amounts, stream);
}

// lgpu_chain_flat_yuv420p_to_yuv: the same without a canvas, ending in lgpu_rgb_to_yuv(.., sink->in_order, 1, .., sink->out_fmt, 0, sink->which_tables); neither RGBA
// frame is written.  Up to 64 tracks as one launch to UYVY / YUYV; to YUV420P 32 per launch (seven pointers per track in the kernel's arguments)
extern "C" int lgpu_chain_flat_yuv420p_to_yuv(const lgpu_chain_params *pr, const lgpu_yuv_source *ys, const lgpu_chain_sink *sk, const lgpu_chain_yuv_sink_track *tracks,
                                              int ntracks, const uint8_t *amounts, void *stream) {
  int rc = ensure_init();
  if (rc) return rc;
  LGPU_REQUIRE(pr && ys && sk && tracks && ntracks > 0 && ntracks <= LGPU_CHAIN_MAX_TRACKS, "params, source, sink and 1..64 tracks required");
  FlatTrack tr[LGPU_CHAIN_MAX_TRACKS];
  flat_sink_tracks(tr, tracks, ntracks);
  return flat_run("lgpu_chain_flat_yuv420p_to_yuv", pr, flat_layer(ys), nullptr, nullptr, sk, tr, ntracks, amounts, stream);
}

// lgpu_chain_flat_yuv420p_mix: lgpu_yuv420p_to_rgb on each track's layer-2 planes (opsize 4, src2's settings, no LUT) + lgpu_chain_flat_yuv420p[_to_yuv] with that
// frame as layer 2, as ONE launch per LGPU_CHAIN_MIX_TRACKS tracks and with no RGBA frame anywhere; every argument is checked before anything is enqueued
extern "C" int lgpu_chain_flat_yuv420p_mix(const lgpu_chain_params *pr, const lgpu_yuv_source *ys, const lgpu_yuv_source *ys2, const lgpu_chain_sink *sk,
                                           const lgpu_chain_yuv_mix_track *tracks, int ntracks, const uint8_t *amounts, void *stream) {
  int rc = ensure_init();
  if (rc) return rc;
  LGPU_REQUIRE(pr && ys && ys2 && tracks && ntracks > 0 && ntracks <= LGPU_CHAIN_MAX_TRACKS, "params, both sources and 1..64 tracks required");
  FlatTrack tr[LGPU_CHAIN_MAX_TRACKS];
  flat_tracks(tr, tracks, ntracks, false);
  const FlatLayer l2 = flat_layer(ys2);
  return flat_run("lgpu_chain_flat_yuv420p_mix", pr, flat_layer(ys), &l2, nullptr, sk, tr, ntracks, amounts, stream);
}

// lgpu_chain_flat_yuv422: lgpu_yuv420p_to_rgb (is_422) or lgpu_yuv_to_rgb (UYVY / YUYV) + lgpu_chain_amounts with sw == dw, sh == dh [+ lgpu_rgb_to_yuv] as ONE launch
// per 64 tracks (32 to YUV420P); every argument is checked before anything is enqueued
extern "C" int lgpu_chain_flat_yuv422(const lgpu_chain_params *pr, const lgpu_yuv422_source *s4, const lgpu_canvas *cv, const lgpu_chain_sink *sk,
                                      const lgpu_chain_yuv_sink_track *tracks, int ntracks, const uint8_t *amounts, void *stream) {
  int rc = ensure_init();
  if (rc) return rc;
  LGPU_REQUIRE(pr && s4 && tracks && ntracks > 0 && ntracks <= LGPU_CHAIN_MAX_TRACKS, "params, source and 1..64 tracks required");
  LGPU_REQUIRE(s4->in_fmt == 2 || s4->in_fmt == 3 || s4->in_fmt == 5, "in_fmt must be 2 (UYVY), 3 (YUYV) or 5 (YUV422P); YUV420P: lgpu_chain_flat_yuv420p[_to_yuv]");
  LGPU_REQUIRE(!(cv && sk), "a canvas and a sink together: chroma rows would straddle the bar / frame edge");
  FlatTrack tr[LGPU_CHAIN_MAX_TRACKS];
  flat_sink_tracks(tr, tracks, ntracks);
  return flat_run("lgpu_chain_flat_yuv422", pr, flat_layer(s4), nullptr, cv, sk, tr, ntracks, amounts, stream);
}

// lgpu_chain_flat_yuv_mix: each track's layer 2 converted by the single-frame call of ITS format (lgpu_yuv420p_to_rgb with is_422 0 / 1, lgpu_yuv_to_rgb) into a tight
// RGBA frame + the one-launch form of layer 1's format with that frame as layer 2, as ONE launch per LGPU_CHAIN_MIX_TRACKS tracks and with no RGBA frame anywhere;
// every argument is checked before anything is enqueued.  With in_fmt 4 on both layers it is lgpu_chain_flat_yuv420p_mix, the same six instantiations.
// lgpu_chain_flat_yuv_mix_canvas: the same with both layers letterboxed onto one canvas (cv, RGBA only), the bars written by the same launch
static int flat_mix(const char *fn, const lgpu_chain_params *pr, const lgpu_yuv_layer_source *s1, const lgpu_yuv_layer_source *s2, const lgpu_canvas *cv,
                    const lgpu_chain_sink *sk, const lgpu_chain_yuv_mix_track *tracks, int ntracks, const uint8_t *amounts, void *stream) {
  int rc = ensure_init();
  if (rc) return rc;
#define MIX_REQUIRE(cond, msg) do { if (!(cond)) { set_error("%s: %s", fn, msg); return LGPU_E_BADARG; } } while (0)
  MIX_REQUIRE(pr && s1 && s2 && tracks && ntracks > 0 && ntracks <= LGPU_CHAIN_MAX_TRACKS, "params, both sources and 1..64 tracks required");
  MIX_REQUIRE(s1->in_fmt >= 2 && s1->in_fmt <= 5 && s2->in_fmt >= 2 && s2->in_fmt <= 5, "in_fmt must be 2 (UYVY), 3 (YUYV), 4 (YUV420P) or 5 (YUV422P) on either layer");
#undef MIX_REQUIRE
  const FlatLayer l1 = flat_layer(s1), l2 = flat_layer(s2);
  FlatTrack tr[LGPU_CHAIN_MAX_TRACKS];
  flat_tracks(tr, tracks, ntracks, l1.packed);
  return flat_run(fn, pr, l1, &l2, cv, sk, tr, ntracks, amounts, stream);
}
extern "C" int lgpu_chain_flat_yuv_mix(const lgpu_chain_params *pr, const lgpu_yuv_layer_source *s1, const lgpu_yuv_layer_source *s2, const lgpu_chain_sink *sk,
                                       const lgpu_chain_yuv_mix_track *tracks, int ntracks, const uint8_t *amounts, void *stream) {
  return flat_mix("lgpu_chain_flat_yuv_mix", pr, s1, s2, nullptr, sk, tracks, ntracks, amounts, stream);
}
extern "C" int lgpu_chain_flat_yuv_mix_canvas(const lgpu_chain_params *pr, const lgpu_yuv_layer_source *s1, const lgpu_yuv_layer_source *s2, const lgpu_canvas *cv,
                                              const lgpu_chain_yuv_mix_track *tracks, int ntracks, const uint8_t *amounts, void *stream) {
  return flat_mix("lgpu_chain_flat_yuv_mix_canvas", pr, s1, s2, cv, nullptr, tracks, ntracks, amounts, stream);
}
