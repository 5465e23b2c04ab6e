// flat_luma.hip -- a LUMA OVERLAY between two decoded frames in one launch (lgpu_chain_flat_yuv_luma, include/lives_gpu_luma.h): luma overlay, underlay, negative overlay
// and averaged overlay of simple_blend.c:151-194 on two YUV420P / YUV422P / UYVY / YUYV layers:
// conversion of the KEYED layer -> [R <-> B] [-> letterbox onto opaque black] -> luma predicate -> conversion of the other layer where it is shown -> select
// [-> gamma LUT] -> RGBA, or -> K4's conversion to UYVY / YUYV / YUV420P.
//
// flat_select.hip's idea with a predicate that comes from data, not from coordinates.  The predicate (luma_pred.h, the one effects.hip's LumaBlend takes) reads ONE
// layer's luma: layer 1's for types 1, 3 and 4, layer 2's for type 2.  That layer is K, the keyed layer, and every cell converts it; O is the other layer.  Both
// finish in the chain's byte order with alpha 255, so the kernel is symmetric in them and the host swaps the roles for type 2: each walk stands in the code once.
// A lane owns the cell (unit, k) of flat.hip's unit walk, converts K's two or four pixels (flat_walk.h), takes their luma from the staged table and decides; then O's
// loads and walk run under a WAVE-UNIFORM condition, a vote over the wave: only if some lane of the wave shows an O pixel.  A wave whose cells all show K issues no load
// of O's planes and none of its table gathers; at threshold 0 no wave of the launch does.  The finished pixel takes flat_select.hip's path: LUT, store or K4; the 4:2:0
// sink's chroma comes from whichever layers' pixels the row pair shows.  The host side -- layer description, track record, refusal sequence, launch shape, dispatch --
// is flat_plan.h's, behind the overlay's own checks (key, type, thresholds).
//
// The bars of a canvas are select(black, black) = opaque black [-> LUT], written by the same launch with nothing read for them.
//
// Per-track data: the threshold travels in the kernel arguments with the nine plane pointers: 32 tracks per launch (LGPU_CHAIN_LUMA_TRACKS), 33..64 as two launches.
#include "lgpu_common.h"
#include "../../include/lives_gpu_luma.h"
#include "k2_walk.h"
#include "flat_walk.h"
#include "flat_plan.h"      // the host side every unscaled form shares: layer description, track record, refusal sequence, launch shape, dispatch
#include "luma_pred.h"
#include <algorithm>
#include <string.h>

namespace lgpu {

struct LumaLayer {
  const int32_t *tables;         // device [5][256] RGB_Y R_Cr G_Cb G_Cr B_Cb (O: null when K's staged copy serves both)
  uint32_t usize, vsize;         // chroma plane bytes; K2's read one past the last row's end is clamped to the last byte of THIS layer's plane
  int ys, us, vs;
  int clamped, lowq, fix_edges;
  int sfmt;                      // packed: 2 UYVY, 3 YUYV (wave-uniform)
};
struct LumaArgs {
  LumaLayer lk, lo;              // the keyed layer and the other one
  const uint2 *stab;             // sink: device [2][3][256] (get_sink_tables)
  const int32_t *luma;           // device [3][256] (DeviceTables::luma)
  int w, h;                      // the frame
  int orow, urow, vrow;          // destination (RGBA / packed / luma) and 4:2:0 chroma rowstrides
  int cw, ch, ox, oy;            // canvas (cw == 0: none)
  int use_lut, fmt, unclamped;   // sink: 2 UYVY, 3 YUYV, 4 YUV420P
  int gy_units, per;             // blockIdx.y < gy_units: the workgroup walks units [y * per, (y + 1) * per); the others write the canvas's bars
  int mode;                      // wave-uniform.  1: show O where luma(K) < t; 3: show O where luma(K) > 255 - t; 2: show K where luma(K) > 255 - t (K is layer 2)
};
template <int NDST> struct LumaTracksT {
  const uint8_t *yk[LGPU_CHAIN_LUMA_TRACKS], *uk[LGPU_CHAIN_LUMA_TRACKS], *vk[LGPU_CHAIN_LUMA_TRACKS];
  const uint8_t *yo[LGPU_CHAIN_LUMA_TRACKS], *uo[LGPU_CHAIN_LUMA_TRACKS], *vo[LGPU_CHAIN_LUMA_TRACKS];
  uint8_t *dst[NDST][LGPU_CHAIN_LUMA_TRACKS];
  uint8_t thr[LGPU_CHAIN_LUMA_TRACKS];
};
template <int SINK> struct LumaSinkLds { uint2 t[6 * 256]; };
template <> struct LumaSinkLds<0> {};
static_assert(sizeof(LumaArgs) + sizeof(LumaTracksT<1>) + sizeof(Lut8) <= 4096 && sizeof(LumaArgs) + sizeof(LumaTracksT<3>) + sizeof(Lut8) <= 4096,
              "HIP documents 4 KB of arguments for a __global__ function");

// SINK: 0 RGBA, 1 packed 4:2:2 (UYVY / YUYV), 2 planar 4:2:0.  SWAP: the finished pixel is BGRA (src->out_order ^ params->swap_rb), on both layers; it is the
// pal_order of the luma too.  KSRC / OSRC: each layer's walk -- 0 planar 4:2:0, 1 planar 4:2:2 (YUV422P), 2 packed 4:2:2 (UYVY / YUYV; T.yk / T.yo is the frame, the
// chroma pointers are not read)
template <int SWAP, int SINK, int KSRC, int OSRC>
__global__ __launch_bounds__(256) void k_flat_luma(const LumaArgs A, const LumaTracksT<SINK == 2 ? 3 : 1> T, const Lut8 lut) {
  static_assert(KSRC >= 0 && KSRC <= 2 && OSRC >= 0 && OSRC <= 2 && SINK >= 0 && SINK <= 2, "KSRC / OSRC: 0 4:2:0, 1 YUV422P, 2 packed");
  __shared__ uint32_t s_ty[2][256];
  __shared__ uint2 s_rg[2][256], s_gb[2][256];
  __shared__ int32_t s_luma[768];
  __shared__ __attribute__((aligned(16))) uint8_t s_lut[256];
  __shared__ LumaSinkLds<SINK> s_sink;
  const int tid = threadIdx.x, z = blockIdx.z;
  stage_lut(s_lut, lut);
  if constexpr (SINK == 0) {
    if ((int)blockIdx.y >= A.gy_units) {
      // letterbox bars: both layers are letterboxed onto the same black canvas, so a bar pixel is a choice between black and black = opaque black [-> LUT]; nothing is read
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
    // K2's tables, paired (flat_walk.h).  O's own copy when its table set or its index clamp differs (a packed layer indexes with the sample itself)
    flat_stage_k2(tid, A.lk.tables, A.lk.clamped, s_ty[0], s_rg[0], s_gb[0]);
    if (A.lo.tables) flat_stage_k2(tid, A.lo.tables, A.lo.clamped, s_ty[1], s_rg[1], s_gb[1]);
#pragma unroll
    for (int i = 0; i < 3; i++) s_luma[tid + 256 * i] = A.luma[tid + 256 * i];
    if constexpr (SINK != 0) {
#pragma unroll
      for (int i = 0; i < 6; i++) s_sink.t[tid + 256 * i] = A.stab[tid + 256 * i];
    }
  }
  __syncthreads();
  const int hw = A.w >> 1, H = A.h;
  const int k = (int)blockIdx.x * 256 + tid;
  if (k >= hw) return;           // the vote below is over the lanes that own a cell
  const int npairs = (H - 1) / 2;                            // full row pairs starting at row 1
  const int nunits = 1 + npairs + (((H - 1) & 1) ? 1 : 0);
  const FlatPlanes PK = {T.yk[z], T.uk[z], T.vk[z], A.lk.usize, A.lk.vsize, A.lk.ys, A.lk.us, A.lk.vs, A.lk.lowq, A.lk.fix_edges};
  const FlatPlanes PO = {T.yo[z], T.uo[z], T.vo[z], A.lo.usize, A.lo.vsize, A.lo.ys, A.lo.us, A.lo.vs, A.lo.lowq, A.lo.fix_edges};
  const int own = A.lo.tables != nullptr;      // wave-uniform
  const FlatK2Lds LK = {s_ty[0], s_rg[0], s_gb[0]}, LO = {s_ty[own], s_rg[own], s_gb[own]};
  const uint32_t bf = T.thr[z], neg = 0xFFu - bf;
  // does a finished pixel of K leave its place to O's?  (luma_pred.h; mode 2: K is layer 2 and is the one shown above the threshold)
  auto showsO = [&](uint32_t pk) -> bool {
    const uint32_t l = luma_px(s_luma, pk, SWAP);
    if (A.mode == 1) return LGPU_LUMA_BELOW(l, bf);
    const bool above = LGPU_LUMA_ABOVE(l, neg);
    return A.mode == 2 ? !above : above;
  };
  // the rest of the chain on the two finished pixels of frame row i, then the store (k_flat_select's emit); cu / cv: the clamped U of the first pixel and V of the
  // second (4:2:0 sink)
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
    const bool pair = unit >= 1 && unit <= npairs;
    const int i = unit == 0 ? 0 : pair ? 2 * unit - 1 : H - 1;
    // SWAP | 2: the walks pack their pixels with byte permutes here (flat_walk.h, flat_px: the compiler's v_ashr_pk_u8_i32 behind the selects below)
    uint32_t p[4] = {0u, 0u, 0u, 0u}, q[4] = {0u, 0u, 0u, 0u};
    {
      auto keep = [&](auto, int, int, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) __attribute__((always_inline)) { p[0] = a0; p[1] = a1; p[2] = b0; p[3] = b1; };
      if constexpr (KSRC == 0) flat_cell<SWAP | 2>(PK, LK, unit, k, hw, H, npairs, keep);
      else flat_cell422<SWAP | 2, KSRC>(PK, LK, A.lk.sfmt, unit, k, H, npairs, keep);
    }
    // decide on K's finished pixels: which of the cell's two or four pixels show O
    const bool s0 = showsO(p[0]), s1 = showsO(p[1]);
    const bool s2 = pair ? showsO(p[2]) : s0, s3 = pair ? showsO(p[3]) : s1;
    const bool someO = __any((int)(s0 | s1 | s2 | s3)) != 0;      // wave-uniform
    if (someO) {
      auto keep = [&](auto, int, int, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) __attribute__((always_inline)) { q[0] = a0; q[1] = a1; q[2] = b0; q[3] = b1; };
      if constexpr (OSRC == 0) flat_cell<SWAP | 2>(PO, LO, unit, k, hw, H, npairs, keep);
      else flat_cell422<SWAP | 2, OSRC>(PO, LO, A.lo.sfmt, unit, k, H, npairs, keep);
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

// k_flat_luma's arguments from the plan (flat_plan.h): one function per struct.  lk / lo: the keyed layer and the other one
static LumaArgs luma_args(const FlatPlan &p, const FlatLayer &lk, const FlatLayer &lo, int type) {
  LumaArgs a;
  memset(&a, 0, sizeof a);
  flat_fill_layer(a.lk, lk);
  flat_fill_layer(a.lo, lo);
  if (flat_tables_shared(lk, lo)) a.lo.tables = nullptr;
  flat_fill_frame(a, p);
  a.luma = device_tables()->luma;
  a.mode = type == 4 ? 1 : type;
  return a;
}
// keyed2: layer 2 is the keyed layer (type 2), so the track's two layers change places
template <int NDST> static void luma_fill_tracks(LumaTracksT<NDST> &T, const FlatPlan &p, const FlatTrack *tr, const lgpu_luma_key *key, bool keyed2, int t0, int n) {
  memset(&T, 0, sizeof T);
  for (int i = 0; i < n; i++) {
    const FlatTrack &t = tr[t0 + i];
    if (keyed2) { T.yk[i] = t.y2; T.uk[i] = t.u2; T.vk[i] = t.v2; T.yo[i] = t.y; T.uo[i] = t.u; T.vo[i] = t.v; }
    else { T.yk[i] = t.y; T.uk[i] = t.u; T.vk[i] = t.v; T.yo[i] = t.y2; T.uo[i] = t.u2; T.vo[i] = t.v2; }
    for (int k = 0; k < p.nplanes; k++) T.dst[k][i] = t.dst[k];
    T.thr[i] = key->thresholds[t0 + i];
  }
}

// lgpu_chain_flat_yuv_luma (include/lives_gpu_luma.h): the overlay's own checks -- key, type, thresholds -- then the refusal sequence of every unscaled form
// (flat_plan): LGPU_E_BADARG before LGPU_E_UNSUPPORTED, everything before anything is allocated or enqueued
extern "C" int lgpu_chain_flat_yuv_luma(const lgpu_chain_params *pr, const lgpu_yuv_layer_source *s1, const lgpu_yuv_layer_source *s2, const lgpu_luma_key *key,
                                        const lgpu_canvas *cv, const lgpu_chain_sink *sk, const lgpu_chain_yuv_mix_track *tracks, int ntracks, void *stream) {
  int rc = ensure_init();
  if (rc) return rc;
  LGPU_REQUIRE(pr && s1 && s2 && key && tracks && ntracks > 0 && ntracks <= LGPU_CHAIN_MAX_TRACKS, "params, both sources, the key and 1..64 tracks required");
  LGPU_REQUIRE(s1->in_fmt >= 2 && s1->in_fmt <= 5 && s2->in_fmt >= 2 && s2->in_fmt <= 5, "in_fmt must be 2 (UYVY), 3 (YUYV), 4 (YUV420P) or 5 (YUV422P) on either layer");
  LGPU_REQUIRE(!(cv && sk), "a canvas and a sink together: chroma rows would straddle the bar / frame edge");
  const int type = key->type;
  LGPU_REQUIRE(type >= 1 && type <= 4, "type must be 1 (overlay), 2 (underlay), 3 (negative overlay) or 4 (averaged overlay)");
  LGPU_REQUIRE(key->thresholds, "null thresholds");
  const FlatLayer l1 = flat_layer(s1), l2 = flat_layer(s2);
  FlatTrack tr[LGPU_CHAIN_MAX_TRACKS];
  flat_tracks(tr, tracks, ntracks, l1.packed);
  FlatPlan p;
  if ((rc = flat_plan("lgpu_chain_flat_yuv_luma", true, "frames that keep their size only (sw == dw, sh == dh)", pr, l1, &l2, cv, sk, tr, ntracks, nullptr, &p))) return rc;
  // the keyed layer is always converted; both layers finish in the chain's order, so the kernel does not know which one is layer 1
  const bool keyed2 = luma_keyed_layer(type) == 2;
  const FlatLayer &lk = keyed2 ? l2 : l1, &lo = keyed2 ? l1 : l2;
  LumaArgs a = luma_args(p, lk, lo, type);
  hipStream_t st = (hipStream_t)stream;
  for (int t0 = 0; t0 < ntracks; t0 += LGPU_CHAIN_LUMA_TRACKS) {
    const int n = std::min(LGPU_CHAIN_LUMA_TRACKS, ntracks - t0);
    const FlatShape s = flat_launch_shape(p, n);
    a.per = s.per; a.gy_units = s.gy_units;
    // THE dispatch point: 3 sinks x KSRC x OSRC x SWAP
    with_constant<3>(p.sink, [&](auto sink) { with_constant<3>(lk.policy, [&](auto ksrc) { with_constant<3>(lo.policy, [&](auto osrc) { with_constant<2>(p.chain_order, [&](auto swap) {
      constexpr int SK = decltype(sink)::value;
      LumaTracksT<SK == 2 ? 3 : 1> T;
      luma_fill_tracks(T, p, tr, key, keyed2, t0, n);
      hipLaunchKernelGGL((k_flat_luma<decltype(swap)::value, SK, decltype(ksrc)::value, decltype(osrc)::value>), s.grid, dim3(256), 0, st, a, T, p.lut);
    }); }); }); });
    LGPU_CHECK_LAUNCH();
  }
  return LGPU_OK;
}
