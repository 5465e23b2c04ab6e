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
#include "lgpu_common.h"
#include "k2_walk.h"
#include "flat_walk.h"      // flat_cell, flat_row422, flat_cell422: the per-cell conversions, shared with flat_select.hip
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
template <int NT, int NDST> static inline void set_sfmt2(FlatMixTracksT<NT, NDST> &, int) {}
template <int NT, int NDST> static inline void set_sfmt2(FlatMixTracksPackedT<NT, NDST> &T, int sfmt2) { T.sfmt2 = sfmt2; }
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
        int q = (int)p, x, y;
        if (q < top) { y = q / A.cw; x = q - y * A.cw; }
        else if (q < top + bottom) { q -= top; y = q / A.cw; x = q - y * A.cw; y += A.oy + A.h; }
        else { q -= top + bottom; y = q / sw_; x = q - y * sw_; y += A.oy; if (x >= A.ox) x += A.w; }
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
    // K2's tables, paired: the entry of an UNCLAMPED blended chroma value e is tables[clamp(e)] (CLAMP16_240 is 16 below 16 and 240 from 0xF0 up on 0..255)
    const int clo = A.clamped ? 16 : 0, chi = A.clamped ? 240 : 255;
    const int ec = tid < clo ? clo : tid > chi ? chi : tid;
    s_ty[tid] = (uint32_t)A.tables[tid];
    s_rg[tid] = make_uint2((uint32_t)A.tables[256 + ec], (uint32_t)A.tables[768 + ec]);
    s_gb[tid] = make_uint2((uint32_t)A.tables[512 + ec], (uint32_t)A.tables[1024 + ec]);
    if constexpr (SINK != 0) {
#pragma unroll
      for (int i = 0; i < 6; i++) s_sink.t[tid + 256 * i] = A.stab[tid + 256 * i];
    }
    if constexpr (L2YUV) {
      if (T.tables2) {        // layer 2's own tables, its own chroma clamp in the index
        const int clo2 = T.clamped2 ? 16 : 0, chi2 = T.clamped2 ? 240 : 255;
        const int e2 = tid < clo2 ? clo2 : tid > chi2 ? chi2 : tid;
        s_l2.ty[tid] = (uint32_t)T.tables2[tid];
        s_l2.rg[tid] = make_uint2((uint32_t)T.tables2[256 + e2], (uint32_t)T.tables2[768 + e2]);
        s_l2.gb[tid] = make_uint2((uint32_t)T.tables2[512 + e2], (uint32_t)T.tables2[1024 + e2]);
      }
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

// all six entry points: tracks in the sink form's layout (the RGBA form's destination is dst_d[0]); cv or sk is null.  ys2 / mix: the second source and the
// caller's tracks of the mix forms (layer 2's planes are read from them; tracks[].layer2_d is null then), null otherwise; with cv both layers are letterboxed onto it.  sfmt / sfmt2: each layer's format,
// 4 planar 4:2:0, 5 planar 4:2:2, 2 UYVY, 3 YUYV (a packed frame is y_d / y2_d with rowstride istrides[0]; the entry points zero the rest of its source)
static int flat_impl(const char *fn, const lgpu_chain_params *pr, const lgpu_yuv_source *ys, const lgpu_canvas *cv, const lgpu_chain_sink *sk,
                     const lgpu_chain_yuv_sink_track *tracks, int ntracks, const uint8_t *amounts, void *stream, const lgpu_yuv_source *ys2 = nullptr,
                     const lgpu_chain_yuv_mix_track *mix = nullptr, int sfmt = 4, int sfmt2 = 4) {
#define FLAT_REQUIRE(cond, msg) do { if (!(cond)) { set_error("%s: %s", fn, msg); return LGPU_E_BADARG; } } while (0)
#define FLAT_REFUSE(msg) do { set_error("%s: %s", fn, msg); return LGPU_E_UNSUPPORTED; } while (0)
  const bool noblend = (pr->interp & LGPU_INTERP_NOBLEND) != 0;
  const bool l2rgba = !noblend && !ys2;      // layer 2 is an RGBA frame of rowstride params->irow2
  FLAT_REQUIRE(pr->interp & LGPU_INTERP_PIXBUF, "the gdk-pixbuf arithmetic only (LGPU_INTERP_PIXBUF)");
  FLAT_REQUIRE(!ys2 || !noblend, "LGPU_INTERP_NOBLEND leaves nothing to mix: lgpu_chain_flat_yuv420p[_to_yuv]");
  FLAT_REQUIRE(amounts || noblend, "null amounts");
  const bool packed = sfmt == 2 || sfmt == 3;
  const int srcp = packed ? 2 : sfmt == 5 ? 1 : 0;      // the kernel's SRC policy
  const bool packed2 = ys2 && (sfmt2 == 2 || sfmt2 == 3);
  const int l2p = !ys2 ? 0 : packed2 ? 3 : sfmt2 == 5 ? 2 : 1;      // the kernel's L2YUV policy
  const int hw = pr->sw >> 1, lys = ys->istrides[0], us = packed ? 0 : ys->istrides[1], vs = packed ? 0 : ys->istrides[2];
  const long usz = packed ? 0 : ys->u_size, vsz = packed ? 0 : ys->v_size;
  int rc;
  if ((rc = check_yuv_source(fn, pr, ys, sfmt)) || (ys2 && (rc = check_yuv_source(fn, pr, ys2, sfmt2)))) return rc;
  const int chain_order = (ys->out_order ^ (pr->swap_rb ? 1 : 0)) & 1;
  FLAT_REQUIRE(!ys2 || ys2->out_order == chain_order, "src2->out_order must state the byte order the blend works in: src->out_order ^ params->swap_rb");
  const bool planar = sk && sk->out_fmt >= 4;
  const int nplanes = planar ? 3 : 1;
  const int cw = cv && !sk ? cv->nwidth : pr->dw, ch = cv && !sk ? cv->nheight : pr->dh;
  if ((rc = sk ? check_yuv_sink(fn, pr, sk, chain_order, l2rgba) : check_rgba_dest(fn, pr, cv, l2rgba))) return rc;
  uintptr_t pb = 0, sb = 0, sb2 = 0;
  for (int i = 0; i < ntracks; i++) {
    const lgpu_chain_yuv_sink_track &t = tracks[i];
    const uint8_t *const planes[3] = {t.y_d, t.u_d, t.v_d};
    if ((rc = check_track(fn, planes, packed ? 1 : 3, false, t.layer2_d, l2rgba, t.dst_d, nplanes, !sk))) return rc;
    sb |= (uintptr_t)t.y_d;
    if (mix) {
      // a packed layer 2 is y2_d alone: its chroma pointers are not read, so they may be null and are no plane a destination could collide with
      const uint8_t *const u2 = packed2 ? nullptr : mix[i].u2_d, *const v2 = packed2 ? nullptr : mix[i].v2_d;
      FLAT_REQUIRE(mix[i].y2_d && (packed2 || (u2 && v2)), "null layer-2 plane");
      for (int k = 0; k < nplanes; k++)
        FLAT_REQUIRE((const uint8_t *)t.dst_d[k] != mix[i].y2_d && (const uint8_t *)t.dst_d[k] != u2 && (const uint8_t *)t.dst_d[k] != v2,
                     "a destination plane is one of layer 2's planes");
      sb2 |= (uintptr_t)mix[i].y2_d;
    }
    pb |= (uintptr_t)t.dst_d[0];
  }
  // the one-launch form; anything else is refused, never run some other way
  if (pr->sw != pr->dw || pr->sh != pr->dh)
    FLAT_REFUSE(srcp ? "frames that keep their size only (sw == dw, sh == dh); convert with lgpu_yuv420p_to_rgb_batch (is_422) / lgpu_yuv_to_rgb_batch and run lgpu_chain_amounts"
                : sk ? "frames that keep their size only (sw == dw, sh == dh); the exact 2:1 reduction is lgpu_chain_yuv420p_to_yuv"
                   : "frames that keep their size only (sw == dw, sh == dh); the exact 2:1 reduction is lgpu_chain_yuv420p");
  if (pr->do_blur) FLAT_REFUSE("the gaussian is not offered with a 4:2:0 or 4:2:2 source");
  // K3 reads a macropixel as one aligned dword; the reference divides that rowstride by 4 (docs/QUIRKS.md, K3-c): there is no behaviour to follow elsewhere
  if (packed && !multiple_of(sb | (uintptr_t)lys, 4)) FLAT_REFUSE("a UYVY / YUYV source is read as 4-byte macropixels (plane and rowstride % 4 == 0)");
  if (packed2 && !multiple_of(sb2 | (uintptr_t)ys2->istrides[0], 4)) FLAT_REFUSE("a UYVY / YUYV layer 2 is read as 4-byte macropixels (plane and rowstride % 4 == 0)");
  if (sk) {
    if (sk->out_fmt == 5) FLAT_REFUSE("YUV422P is not served (lgpu_chain_flat_yuv420p + lgpu_rgb_to_yuv_batch)");
    if (planar && (pr->dh & 1)) FLAT_REFUSE("the 4:2:0 sink needs an even height");
    // a lane stores one macropixel (4 bytes) or one luma pair (2 bytes) per row; chroma samples are single bytes
    if (!multiple_of(pb | (uintptr_t)sk->orow[0], planar ? 2 : 4))
      FLAT_REFUSE("packed sinks are stored as 4-byte macropixels (plane and rowstride % 4 == 0), the 4:2:0 luma plane as 2-byte pairs (plane and rowstride % 2 == 0)");
  }
  const int drow = sk ? sk->orow[0] : pr->orow;
  if ((rc = check_plane_sizes(fn, {(long long)pr->sh * lys, usz, vsz, (long long)ch * drow, l2rgba ? (long long)ch * pr->irow2 : 0,
                                   ys2 ? (long long)pr->sh * ys2->istrides[0] : 0, ys2 ? ys2->u_size : 0, ys2 ? ys2->v_size : 0,
                                   planar ? (long long)(pr->dh >> 1) * sk->orow[1] : 0, planar ? (long long)(pr->dh >> 1) * sk->orow[2] : 0}))) return rc;
  FlatArgs a;
  memset(&a, 0, sizeof a);
  if (planar && (rc = cavg_forms_checked())) return rc;
  if (sk && (rc = get_sink_tables(sk->which_tables, sk->in_order, &a.stab))) return rc;
  a.tables = device_tables()->yuv2rgb[ys->which_tables & 3];
  a.usize = (uint32_t)usz; a.vsize = (uint32_t)vsz; a.ys = lys; a.us = us; a.vs = vs; a.w = pr->sw; a.h = pr->sh;
  a.orow = drow; a.irow2 = l2rgba ? pr->irow2 : 0;
  a.urow = planar ? sk->orow[1] : 0; a.vrow = planar ? sk->orow[2] : 0;
  if (cv) { a.cw = cv->nwidth; a.ch = cv->nheight; a.ox = cv->offs_x; a.oy = cv->offs_y; }
  a.clamped = !packed && !(ys->which_tables & 1);      // K3 indexes its tables with the sample itself
  a.sfmt = packed ? sfmt : 0;
  a.lowq = ys->pb_quality == 1; a.fix_edges = (ys->flags & LGPU_YUV_FIX_EDGES) ? 1 : 0; a.use_lut = pr->use_lut ? 1 : 0;
  a.fmt = sk ? sk->out_fmt : 0; a.unclamped = sk ? (sk->which_tables & 1) : 0;
  const Lut8 l = pack_lut(pr->use_lut ? pr->lut8 : nullptr);
  const int nunits = pr->sh / 2 + 1;
  const unsigned gx = cdiv((unsigned)hw, 256u);
  const long long bar_px = cv ? (long long)cw * ch - (long long)pr->sw * pr->sh : 0;
  const int per_launch = ys2 ? LGPU_CHAIN_MIX_TRACKS : planar ? kFlatPlanarTracks : LGPU_CHAIN_MAX_TRACKS;
  hipStream_t st = (hipStream_t)stream;
#define FLAT_LAUNCH_SRC(SK, SR) do {                                                                                                                     \
    if (noblend) { if (chain_order) hipLaunchKernelGGL((k_flat_yuv420<0, 1, SK, 0, SR>), grid, dim3(256), 0, st, a, T, l); else hipLaunchKernelGGL((k_flat_yuv420<0, 0, SK, 0, SR>), grid, dim3(256), 0, st, a, T, l); } \
    else { if (chain_order) hipLaunchKernelGGL((k_flat_yuv420<1, 1, SK, 0, SR>), grid, dim3(256), 0, st, a, T, l); else hipLaunchKernelGGL((k_flat_yuv420<1, 0, SK, 0, SR>), grid, dim3(256), 0, st, a, T, l); }     \
  } while (0)
#define FLAT_LAUNCH(SK) do { if (srcp == 2) FLAT_LAUNCH_SRC(SK, 2); else if (srcp == 1) FLAT_LAUNCH_SRC(SK, 1); else FLAT_LAUNCH_SRC(SK, 0); } while (0)
  for (int t0 = 0; t0 < ntracks; t0 += per_launch) {
    const int n = std::min(per_launch, ntracks - t0);
    // about kFlatWgTarget workgroups per launch, each walking a run of consecutive units on one staging of the tables
    const int cap = std::max(1, (int)(kFlatWgTarget / ((long long)gx * n)));
    int gy = std::min(nunits, cap);
    a.per = (nunits + gy - 1) / gy;
    gy = (nunits + a.per - 1) / a.per;
    a.gy_units = gy;
    const unsigned bar_gy = bar_px > 0 ? (unsigned)std::min<long long>(64, (bar_px + 1024ll * gx - 1) / (1024ll * gx)) : 0u;
    const dim3 grid(gx, (unsigned)gy + bar_gy, (unsigned)n);
    if (ys2) {
      // L2YUV: one staged copy of the K2 tables serves both layers when they index the same set the same way.  A planar layer with clamped tables indexes rg / gb
      // through the 16..240 clamp that staging folds into the index, a packed layer with the sample itself: UYVY over YUV420P, both with which_tables 0, needs two copies
      const int clamped2 = !packed2 && !(ys2->which_tables & 1);
      const bool own = (ys2->which_tables & 3) != (ys->which_tables & 3) || clamped2 != a.clamped;
      auto fill = [&](auto &T) {
        for (int i = 0; i < n; i++) {
          const lgpu_chain_yuv_mix_track &t = mix[t0 + i];
          T.y[i] = t.y_d; T.u[i] = t.u_d; T.v[i] = t.v_d; T.y2[i] = t.y2_d; T.u2[i] = t.u2_d; T.v2[i] = t.v2_d; T.bf[i] = amounts[t0 + i];
          for (int k = 0; k < nplanes; k++) T.dst[k][i] = t.dst_d[k];
        }
        T.tables2 = own ? device_tables()->yuv2rgb[ys2->which_tables & 3] : nullptr;
        T.usize2 = (uint32_t)ys2->u_size; T.vsize2 = (uint32_t)ys2->v_size; T.ys2 = ys2->istrides[0]; T.us2 = ys2->istrides[1]; T.vs2 = ys2->istrides[2];
        T.clamped2 = clamped2; T.lowq2 = ys2->pb_quality == 1; T.fix_edges2 = (ys2->flags & LGPU_YUV_FIX_EDGES) ? 1 : 0;
      };
      // THE dispatch point of the mix forms: 3 sinks x SRC x L2YUV x SWAP, the six of lgpu_chain_flat_yuv420p_mix (SRC 0, L2YUV 1) among them
#define FLAT_MIX_LAUNCH_L2(SK, SR, L2) do {                                                                                                  \
        FlatTr<SK, L2>::type T;                                                                                                              \
        memset(&T, 0, sizeof T);                                                                                                             \
        fill(T);                                                                                                                             \
        set_sfmt2(T, sfmt2);                                                                                                                 \
        if (chain_order) hipLaunchKernelGGL((k_flat_yuv420<1, 1, SK, L2, SR>), grid, dim3(256), 0, st, a, T, l);                            \
        else hipLaunchKernelGGL((k_flat_yuv420<1, 0, SK, L2, SR>), grid, dim3(256), 0, st, a, T, l);                                        \
      } while (0)
#define FLAT_MIX_LAUNCH_SRC(SK, SR) do {                                                                                                     \
        if (l2p == 3) FLAT_MIX_LAUNCH_L2(SK, SR, 3); else if (l2p == 2) FLAT_MIX_LAUNCH_L2(SK, SR, 2); else FLAT_MIX_LAUNCH_L2(SK, SR, 1);   \
      } while (0)
#define FLAT_MIX_LAUNCH(SK) do { if (srcp == 2) FLAT_MIX_LAUNCH_SRC(SK, 2); else if (srcp == 1) FLAT_MIX_LAUNCH_SRC(SK, 1); else FLAT_MIX_LAUNCH_SRC(SK, 0); } while (0)
      if (planar) FLAT_MIX_LAUNCH(2); else if (sk) FLAT_MIX_LAUNCH(1); else FLAT_MIX_LAUNCH(0);
#undef FLAT_MIX_LAUNCH
#undef FLAT_MIX_LAUNCH_SRC
#undef FLAT_MIX_LAUNCH_L2
    } else if (planar) {
      FlatTr<2>::type T;
      for (int i = 0; i < n; i++) {
        const lgpu_chain_yuv_sink_track &t = tracks[t0 + i];
        T.y[i] = t.y_d; T.u[i] = t.u_d; T.v[i] = t.v_d; T.l2[i] = noblend ? nullptr : t.layer2_d; T.bf[i] = amounts ? amounts[t0 + i] : 0;
        for (int k = 0; k < 3; k++) T.dst[k][i] = t.dst_d[k];
      }
      FLAT_LAUNCH(2);
    } else {
      FlatTr<0>::type T;
      for (int i = 0; i < n; i++) {
        const lgpu_chain_yuv_sink_track &t = tracks[t0 + i];
        T.y[i] = t.y_d; T.u[i] = t.u_d; T.v[i] = t.v_d; T.l2[i] = noblend ? nullptr : t.layer2_d; T.bf[i] = amounts ? amounts[t0 + i] : 0;
        T.dst[0][i] = t.dst_d[0];
      }
      if (sk) FLAT_LAUNCH(1); else FLAT_LAUNCH(0);
    }
    LGPU_CHECK_LAUNCH();
  }
  return LGPU_OK;
#undef FLAT_LAUNCH
#undef FLAT_LAUNCH_SRC
#undef FLAT_REQUIRE
#undef FLAT_REFUSE
}

// lgpu_chain_flat_yuv420p: lgpu_yuv420p_to_rgb (opsize 4, src->out_order, no LUT) + lgpu_chain_amounts with sw == dw, sh == dh, as ONE launch (the canvas's bars
// included); every argument is checked before anything is enqueued
extern "C" int lgpu_chain_flat_yuv420p(const lgpu_chain_params *pr, const lgpu_yuv_source *ys, const lgpu_canvas *cv, const lgpu_chain_yuv_track *tracks, int ntracks,
                                       const uint8_t *amounts, void *stream) {
  int rc = ensure_init();
  if (rc) return rc;
  LGPU_REQUIRE(pr && ys && tracks && ntracks > 0 && ntracks <= LGPU_CHAIN_MAX_TRACKS, "params, source and 1..64 tracks required");
  lgpu_chain_yuv_sink_track tr[LGPU_CHAIN_MAX_TRACKS];
  for (int i = 0; i < ntracks; i++) {
    tr[i].y_d = tracks[i].y_d; tr[i].u_d = tracks[i].u_d; tr[i].v_d = tracks[i].v_d; tr[i].layer2_d = tracks[i].layer2_d;
    tr[i].dst_d[0] = tracks[i].dst_d; tr[i].dst_d[1] = tr[i].dst_d[2] = nullptr;
  }
  return flat_impl("lgpu_chain_flat_yuv420p", pr, ys, cv, nullptr, tr, ntracks, amounts, stream);
}

// lgpu_chain_flat_yuv420p_to_yuv: the same without a canvas, ending in lgpu_rgb_to_yuv(.., sink->in_order, 1, .., sink->out_fmt, 0, sink->which_tables); neither RGBA
// frame is written.  Up to 64 tracks as one launch to UYVY / YUYV; to YUV420P 32 per launch (seven pointers per track in the kernel's arguments)
extern "C" int lgpu_chain_flat_yuv420p_to_yuv(const lgpu_chain_params *pr, const lgpu_yuv_source *ys, const lgpu_chain_sink *sk, const lgpu_chain_yuv_sink_track *tracks,
                                              int ntracks, const uint8_t *amounts, void *stream) {
  int rc = ensure_init();
  if (rc) return rc;
  LGPU_REQUIRE(pr && ys && sk && tracks && ntracks > 0 && ntracks <= LGPU_CHAIN_MAX_TRACKS, "params, source, sink and 1..64 tracks required");
  return flat_impl("lgpu_chain_flat_yuv420p_to_yuv", pr, ys, nullptr, sk, tracks, ntracks, amounts, stream);
}

// lgpu_chain_flat_yuv420p_mix: lgpu_yuv420p_to_rgb on each track's layer-2 planes (opsize 4, src2's settings, no LUT) + lgpu_chain_flat_yuv420p[_to_yuv] with that
// frame as layer 2, as ONE launch per LGPU_CHAIN_MIX_TRACKS tracks and with no RGBA frame anywhere; every argument is checked before anything is enqueued
extern "C" int lgpu_chain_flat_yuv420p_mix(const lgpu_chain_params *pr, const lgpu_yuv_source *ys, const lgpu_yuv_source *ys2, const lgpu_chain_sink *sk,
                                           const lgpu_chain_yuv_mix_track *tracks, int ntracks, const uint8_t *amounts, void *stream) {
  int rc = ensure_init();
  if (rc) return rc;
  LGPU_REQUIRE(pr && ys && ys2 && tracks && ntracks > 0 && ntracks <= LGPU_CHAIN_MAX_TRACKS, "params, both sources and 1..64 tracks required");
  lgpu_chain_yuv_sink_track tr[LGPU_CHAIN_MAX_TRACKS];
  for (int i = 0; i < ntracks; i++) {
    tr[i].y_d = tracks[i].y_d; tr[i].u_d = tracks[i].u_d; tr[i].v_d = tracks[i].v_d; tr[i].layer2_d = nullptr;
    for (int k = 0; k < 3; k++) tr[i].dst_d[k] = tracks[i].dst_d[k];
  }
  return flat_impl("lgpu_chain_flat_yuv420p_mix", pr, ys, nullptr, sk, tr, ntracks, amounts, stream, ys2, tracks);
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
  lgpu_yuv_source ys;
  memset(&ys, 0, sizeof ys);
  const bool packed = s4->in_fmt != 5;
  ys.istrides[0] = s4->istrides[0]; ys.istrides[1] = packed ? 0 : s4->istrides[1]; ys.istrides[2] = packed ? 0 : s4->istrides[2];
  ys.u_size = packed ? 0 : s4->u_size; ys.v_size = packed ? 0 : s4->v_size;
  ys.out_order = s4->out_order; ys.which_tables = s4->which_tables; ys.pb_quality = s4->pb_quality;
  return flat_impl("lgpu_chain_flat_yuv422", pr, &ys, cv, sk, tracks, ntracks, amounts, stream, nullptr, nullptr, s4->in_fmt);
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
  // one layer's description as flat_impl reads it; what a packed layer does not have is zero
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
  const bool packed1 = s1->in_fmt < 4;
  lgpu_chain_yuv_sink_track tr[LGPU_CHAIN_MAX_TRACKS];
  for (int i = 0; i < ntracks; i++) {
    tr[i].y_d = tracks[i].y_d; tr[i].u_d = packed1 ? nullptr : tracks[i].u_d; tr[i].v_d = packed1 ? nullptr : tracks[i].v_d; tr[i].layer2_d = nullptr;
    for (int k = 0; k < 3; k++) tr[i].dst_d[k] = tracks[i].dst_d[k];
  }
  return flat_impl(fn, pr, &ys, cv, sk, tr, ntracks, amounts, stream, &ys2, tracks, s1->in_fmt, s2->in_fmt);
}
extern "C" int lgpu_chain_flat_yuv_mix(const lgpu_chain_params *pr, const lgpu_yuv_layer_source *s1, const lgpu_yuv_layer_source *s2, const lgpu_chain_sink *sk,
                                       const lgpu_chain_yuv_mix_track *tracks, int ntracks, const uint8_t *amounts, void *stream) {
  return flat_mix("lgpu_chain_flat_yuv_mix", pr, s1, s2, nullptr, sk, tracks, ntracks, amounts, stream);
}
extern "C" int lgpu_chain_flat_yuv_mix_canvas(const lgpu_chain_params *pr, const lgpu_yuv_layer_source *s1, const lgpu_yuv_layer_source *s2, const lgpu_canvas *cv,
                                              const lgpu_chain_yuv_mix_track *tracks, int ntracks, const uint8_t *amounts, void *stream) {
  return flat_mix("lgpu_chain_flat_yuv_mix_canvas", pr, s1, s2, cv, nullptr, tracks, ntracks, amounts, stream);
}
