// flat_walk.h -- the per-cell conversions of the unscaled one-launch forms: a lane's cell (unit, chroma column k) of a decoded YUV420P / YUV422P / UYVY / YUYV frame as
// two or four finished RGBA pixels.  flat.hip's k_flat_yuv420 (one layer, or both layers at every cell: the chroma blend) and flat_select.hip's k_flat_select (the layer
// a pixel SHOWS, decided before anything is loaded) walk the same cells through these functions, so the two forms cannot drift apart.  The staging of K2's paired
// tables (flat_stage_k2) and the decode of a bar pixel (flat_bar_xy) are here for the same reason.  The kernels' host side is flat_plan.h.
#pragma once
#include "lgpu_common.h"
#include "k2_walk.h"

namespace lgpu {

// an address or pitch as a multiple of n (a power of two).  Every alignment decision of flat.hip and flat_select.hip goes through it, in the kernel and in the entry points;
// tests/test_chain_flat.py walks each class they tell apart (test_chain_flat_addresses, test_chain_flat_refusals)
__host__ __device__ static inline bool multiple_of(uintptr_t v, unsigned n) { return v % n == 0; }

// one layer's planes as K2 reads them, and the staged K2 tables they are converted with
struct FlatPlanes {
  const uint8_t *y, *u, *v;
  uint32_t usize, vsize;         // chroma plane bytes; K2's read one past the last row's end is clamped to the last byte of THIS layer's plane
  int ys, us, vs;
  int lowq, fix_edges;
};
struct FlatK2Lds { const uint32_t *ty; const uint2 *rg, *gb; };
template <int KIND> struct FlatCell { static constexpr int value = KIND; };      // 0: row 0, 1: a row pair, 2: the trailing row

// K2's tables, paired, staged into LDS by the workgroup's 256 lanes: the entry of an UNCLAMPED blended chroma value e is tables[clamp(e)] (CLAMP16_240 is 16 below 16
// and 240 from 0xF0 up on 0..255).  clamped: the layer's own chroma clamp in the index (a packed layer indexes with the sample itself).  Every layer of both kernels
// is staged here: layer 2 has its own copy when its table set or its index clamp differs (flat_plan.h, flat_tables_shared)
__device__ __forceinline__ void flat_stage_k2(int tid, const int32_t *tables, int clamped, uint32_t *ty, uint2 *rg, uint2 *gb) {
  const int clo = clamped ? 16 : 0, chi = clamped ? 240 : 255;
  const int ec = tid < clo ? clo : tid > chi ? chi : tid;
  ty[tid] = (uint32_t)tables[tid];
  rg[tid] = make_uint2((uint32_t)tables[256 + ec], (uint32_t)tables[768 + ec]);
  gb[tid] = make_uint2((uint32_t)tables[512 + ec], (uint32_t)tables[1024 + ec]);
}

// pixel q of the canvas's bars as (x, y) on the canvas: the `top` pixels above the frame, the `bottom` ones below it, then the sw = cw - w of each of the frame's h
// rows, left bar and right.  The w x h frame sits at (ox, oy) on a canvas cw wide
__device__ __forceinline__ void flat_bar_xy(int q, int top, int bottom, int sw, int cw, int ox, int oy, int w, int h, int &x, int &y) {
  if (q < top) { y = q / cw; x = q - y * cw; }
  else if (q < top + bottom) { q -= top; y = q / cw; x = q - y * cw; y += oy + h; }
  else { q -= top + bottom; y = q / sw; x = q - y * sw; y += oy; if (x >= ox) x += w; }
}

// xyuv2rgb on the paired tables; the chroma index is the blended value itself.  SWAP & 1: the pixel is BGRA.
// SWAP & 2 (k_flat_select passes SWAP | 2 to the walks below): the same pixel packed with two byte permutes (selector 0x0C = 0x00, 0x0D = 0xFF), as palette.hip's
// k_uyvy_to_rgb_s packs it.  Behind that kernel's selects the compiler fused shift + clamp + pack of the shifts-and-ORs form into v_ashr_pk_u8_i32 with the destination
// among its sources, whose upper result half it takes for zero: the third byte of every second-row pixel came out OR-ed with the second (gfx950, ROCm 7.2;
// tests/test_isa_hazards.py fails on such a use).  k_flat_yuv420 keeps the shifts and ORs: its instantiations have no such use and stay the machine code they were
template <int SWAP>
__device__ __forceinline__ uint32_t flat_px(const FlatK2Lds &L, uint32_t yv, uint32_t iu, uint32_t iv) {
  const uint32_t yy = L.ty[yv];
  const uint2 rg = L.rg[iv], gb = L.gb[iu];
  uint32_t r, g, b;
  yuv_rgb(yy, rg.x, rg.y, gb.x, gb.y, r, g, b);
  if constexpr ((SWAP & 2) != 0)
    return (SWAP & 1) ? __builtin_amdgcn_perm(r, __builtin_amdgcn_perm(g, b, 0x0C0C0400u), 0x0D040100u)
                      : __builtin_amdgcn_perm(b, __builtin_amdgcn_perm(g, r, 0x0C0C0400u), 0x0D040100u);
  return SWAP ? (b | (g << 8) | (r << 16) | 0xFF000000u) : (r | (g << 8) | (b << 16) | 0xFF000000u);
}

// K2's walk (k2_walk.h) for cell (unit, k) of one layer: its two pixels of one row or its 2 x 2 quad go to out(FlatCell<KIND>, first row, chroma row, p0, p1, second row's p0, p1).  Either layer
// of the L2YUV forms comes through here when it is planar 4:2:0, each with its own planes and tables
template <int SWAP, class Out>
__device__ __forceinline__ void flat_cell(const FlatPlanes &P, const FlatK2Lds &L, int unit, int k, int hw, int H, int npairs, Out &&out) {
  const uint8_t *py = P.y, *pu = P.u, *pv = P.v;
  auto PU = [&](int r, int kk) -> uint32_t { long i = (long)r * P.us + kk; return pu[i < (long)P.usize ? i : (long)P.usize - 1]; };
  auto PV = [&](int r, int kk) -> uint32_t { long i = (long)r * P.vs + kk; return pv[i < (long)P.vsize ? i : (long)P.vsize - 1]; };
  auto ld32 = [](const uint8_t *p) -> uint32_t { uint32_t w; __builtin_memcpy(&w, p, 4); return w; };
  auto ld16 = [](const uint8_t *p) -> uint32_t { uint16_t w; __builtin_memcpy(&w, p, 2); return w; };
  auto px = [&](uint32_t yv, uint32_t iu, uint32_t iv) -> uint32_t { return flat_px<SWAP>(L, yv, iu, iv); };
  // K2's vblend: (2a + b) / 3 and (a + 2b) / 3 on doubled sums, or the halves with pb_quality LOW
  auto vtop = [&](uint32_t s1, uint32_t s2) -> uint32_t { return P.lowq ? s1 >> 1 : yuv_third(s1, s2); };
  auto vbot = [&](uint32_t s1, uint32_t s2) -> uint32_t { return P.lowq ? s2 >> 1 : yuv_third(s2, s1); };
  if (unit == 0) {
    const uint32_t yy = ld16(py + 2 * k);
    uint32_t p0, p1;
    k2_row_pixels(k2_row_edge(0, k, hw, PU, PV), yy & 0xFF, yy >> 8, px, p0, p1);
    out(FlatCell<0>(), 0, 0, p0, p1, 0u, 0u);
  } else if (unit <= npairs) {
    // rows (i, i + 1), chroma rows r and r + 1
    const int i = 2 * unit - 1, r = unit - 1;
    const uint32_t ya = ld16(py + (size_t)i * P.ys + 2 * k), yb = ld16(py + (size_t)(i + 1) * P.ys + 2 * k);
    // k2_walk.h's k2_pair_samples + k2_pair_pixels (rules b-f) in this kernel's own text and statement order: through the header two instantiations ran 0.6 % slower
    // (profiles/r18/k2_walk.md)
    uint32_t u_l, u_c, u_n, u1_c, u1_n, v_c, v_n, v1_l, v1_c, v1_n, v1_0;
    const long ou = (long)(r + 1) * P.us, ov = (long)(r + 1) * P.vs;
    if (k >= 1 && ou + k + 3 <= (long)P.usize && ov + k + 3 <= (long)P.vsize) {
      // interior: one 4-byte window (columns k - 1 .. k + 2, the last unused) per chroma row
      const uint32_t wu0 = ld32(pu + (ou - P.us + k - 1)), wu1 = ld32(pu + (ou + k - 1)), wv0 = ld32(pv + (ov - P.vs + k - 1)), wv1 = ld32(pv + (ov + k - 1));
      v1_0 = pv[ov];
      u_l = wu0 & 0xFF; u_c = (wu0 >> 8) & 0xFF; u_n = (wu0 >> 16) & 0xFF; u1_c = (wu1 >> 8) & 0xFF; u1_n = (wu1 >> 16) & 0xFF;
      v_c = (wv0 >> 8) & 0xFF; v_n = (wv0 >> 16) & 0xFF; v1_l = wv1 & 0xFF; v1_c = (wv1 >> 8) & 0xFF; v1_n = (wv1 >> 16) & 0xFF;
    } else {
      u_c = PU(r, k); v_c = PV(r, k); v1_c = PV(r + 1, k);
      u_l = k ? PU(r, k - 1) : u_c;
      v1_l = k ? PV(r + 1, k - 1) : v_c;
      v1_0 = PV(r + 1, 0);
      u_n = PU(r, k + 1); u1_c = PU(r + 1, k); u1_n = PU(r + 1, k + 1);
      v_n = PV(r, k + 1); v1_n = PV(r + 1, k + 1);
    }
    const uint32_t su = u_c + u_l, s1v = v_c + v1_l, s2v = v1_c + v1_0;
    const uint32_t a0 = px(ya & 0xFF, vtop(su, su), vtop(s1v, s2v)), b0 = px(yb & 0xFF, vbot(su, su), vbot(s1v, s2v));
    const uint32_t s1u = u_c + u_n, s2u = u1_c + u1_n, s1w = v_c + v_n, s2w = v1_c + v1_n;
    const uint32_t a1 = px(ya >> 8, vtop(s1u, s2u), vtop(s1w, s2w)), b1 = px(yb >> 8, vbot(s1u, s2u), vbot(s1w, s2w));
    out(FlatCell<1>(), i, r, a0, a1, b0, b1);
  } else {
    // trailing row H - 1
    const int i = H - 1, r = i >> 1;
    // k2_walk.h's k2_trailing_pixels (rules g, h) in this kernel's own text
    const int kp = k ? k - 1 : 0, kn = (k + 1 < hw) ? k + 1 : hw - 1;
    const uint32_t yy = ld16(py + (size_t)i * P.ys + 2 * k), uk = PU(r, k), vk = PV(r, k);
    uint32_t p0;
    if (P.fix_edges) p0 = px(yy & 0xFF, (uk + PU(r, kp)) >> 1, (vk + PV(r, kp)) >> 1);
    else {
      const uint32_t tu = k ? PU(0, k) : PU(r, 0), tv = k ? PV(0, k) : PV(r, 0);
      const uint32_t lu = (k >= 2) ? PU(0, k - 1) : PU(r, 0), lv = (k >= 2) ? PV(0, k - 1) : PV(r, 0);
      p0 = px(py[2 * k], (tu + lu) >> 1, (tv + lv) >> 1);
    }
    const uint32_t p1 = px(yy >> 8, (uk + PU(r, kn)) >> 1, (vk + PV(r, kn)) >> 1);
    out(FlatCell<2>(), i, r, p0, p1, 0u, 0u);
  }
}

// one row's pixel pair of cell k of a 4:2:2 frame (the SRC policies of k_flat_yuv420 for layer 1, L2YUV - 1 for layer 2).
// SRC == 1, planar (YUV422P): K2's 4:2:2 row (k2_walk.h, rules i and e); pb_quality and LGPU_YUV_FIX_EDGES change nothing in this walk.
// SRC == 2, packed (UYVY / YUYV): K3's conversion (palette.hip k_yuv_to_rgb / k_uyvy_to_rgb_s, uyvy2rgb :2410-2415, yuyv2rgb :2418-2423): both pixels of a macropixel
// under its own U and V, no interpolation and no chroma clamp (the host stages the tables with the identity index); one aligned dword per lane and row
template <int SWAP, int SRC>
__device__ __forceinline__ void flat_row422(const FlatPlanes &P, const FlatK2Lds &L, int sfmt, int i, int k, uint32_t &p0, uint32_t &p1) {
  auto px = [&](uint32_t yv, uint32_t iu, uint32_t iv) -> uint32_t { return flat_px<SWAP>(L, yv, iu, iv); };
  if constexpr (SRC == 2) {
    const uint32_t m = *reinterpret_cast<const uint32_t *>(P.y + (size_t)i * P.ys + 4 * (size_t)k);
    uint32_t y0, y1, u, v;
    if (sfmt == 2) { u = m & 0xFF; y0 = (m >> 8) & 0xFF; v = (m >> 16) & 0xFF; y1 = m >> 24; }
    else { y0 = m & 0xFF; u = (m >> 8) & 0xFF; y1 = (m >> 16) & 0xFF; v = m >> 24; }
    p0 = px(y0, u, v); p1 = px(y1, u, v);
  } else {
    const uint8_t *pu = P.u, *pv = P.v;
    auto PU = [&](int r, int kk) -> uint32_t { long q = (long)r * P.us + kk; return pu[q < (long)P.usize ? q : (long)P.usize - 1]; };
    auto PV = [&](int r, int kk) -> uint32_t { long q = (long)r * P.vs + kk; return pv[q < (long)P.vsize ? q : (long)P.vsize - 1]; };
    uint16_t yy;
    __builtin_memcpy(&yy, P.y + (size_t)i * P.ys + 2 * k, 2);
    const long ou = (long)i * P.us + k, ov = (long)i * P.vs + k;
    K2Row<uint32_t> s;
    if (k >= 2 && ou + 3 <= (long)P.usize && ov + 3 <= (long)P.vsize) {
      // interior (no seeded sample from column 2 on): one 4-byte window (columns k - 1 .. k + 2, the last unused) per chroma plane
      uint32_t wu, wv;
      __builtin_memcpy(&wu, pu + (ou - 1), 4); __builtin_memcpy(&wv, pv + (ov - 1), 4);
      s.lu = wu & 0xFF; s.tu = (wu >> 8) & 0xFF; s.nu = (wu >> 16) & 0xFF;
      s.lv = wv & 0xFF; s.tv = (wv >> 8) & 0xFF; s.nv = (wv >> 16) & 0xFF;
    } else {
      // k2_walk.h's k2_row_422 (rules i and e) in this function's own text: through the header four instantiations take one more register
      s.tu = k ? PU(i, k) : PU(i >> 1, 0); s.tv = k ? PV(i, k) : PV(i >> 1, 0);
      s.lu = (k >= 2) ? PU(i, k - 1) : PU(i >> 1, 0); s.lv = (k >= 2) ? PV(i, k - 1) : PV(i >> 1, 0);
      s.nu = PU(i, k + 1); s.nv = PV(i, k + 1);
    }
    k2_row_pixels(s, yy & 0xFFu, (uint32_t)yy >> 8, px, p0, p1);
  }
}

// the unit walk of flat_cell over a 4:2:2 frame: the same cells go to out() -- row 0, a row pair, the trailing row -- each row converted on its own
template <int SWAP, int SRC, class Out>
__device__ __forceinline__ void flat_cell422(const FlatPlanes &P, const FlatK2Lds &L, int sfmt, int unit, int k, int H, int npairs, Out &&out) {
  uint32_t a0, a1, b0, b1;
  if (unit == 0) {
    flat_row422<SWAP, SRC>(P, L, sfmt, 0, k, a0, a1);
    out(FlatCell<0>(), 0, 0, a0, a1, 0u, 0u);
  } else if (unit <= npairs) {
    const int i = 2 * unit - 1;
    flat_row422<SWAP, SRC>(P, L, sfmt, i, k, a0, a1);
    flat_row422<SWAP, SRC>(P, L, sfmt, i + 1, k, b0, b1);
    out(FlatCell<1>(), i, unit - 1, a0, a1, b0, b1);
  } else {
    flat_row422<SWAP, SRC>(P, L, sfmt, H - 1, k, a0, a1);
    out(FlatCell<2>(), H - 1, (H - 1) >> 1, a0, a1, 0u, 0u);
  }
}

// K4 on the two finished pixels of one row (k_pb_half's sink_row): the nine table sums >> 16 as a short, upper clamp then lower (k_flat_yuv420's emit keeps these
// lines in its own text, so that its instantiations stay the machine code they were; k_flat_select calls this).  t: the staged {Y, U} / {Y, V}
// tables of get_sink_tables.  y0c / y1c: the clamped lumas; ur / vr: U of the first pixel and V of the second, not yet clamped (rgb2yuyv lost its upper clamp)
__device__ __forceinline__ void flat_k4_pair(const uint2 *t, int unclamped, uint32_t p0, uint32_t p1, uint32_t &y0c, uint32_t &y1c, int &ur, int &vr) {
  const uint2 *tu = t, *tv = t + 768;
  const uint2 a0 = tu[p0 & 0xFF], b0 = tu[256 + ((p0 >> 8) & 0xFF)], c0 = tu[512 + ((p0 >> 16) & 0xFF)];
  const uint2 a1 = tv[p1 & 0xFF], b1 = tv[256 + ((p1 >> 8) & 0xFF)], c1 = tv[512 + ((p1 >> 16) & 0xFF)];
  const int min_y = unclamped ? 0 : 16, max_y = unclamped ? 255 : 235;
  const int ya = (int)(a0.x + b0.x + c0.x) >> 16, yb = (int)(a1.x + b1.x + c1.x) >> 16;
  ur = (int)(a0.y + b0.y + c0.y) >> 16; vr = (int)(a1.y + b1.y + c1.y) >> 16;
  y0c = (uint32_t)min(max(ya, min_y), max_y); y1c = (uint32_t)min(max(yb, min_y), max_y);
}

}  // namespace lgpu
