// lgpu_common.h -- shared device helpers / launch plumbing for liblivesgpu.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <initializer_list>
#include "../../include/lives_gpu.h"

namespace lgpu {

// ---- error plumbing -------------------------------------------------------------------------------
void set_error(const char *fmt, ...);
int ensure_init();   // LGPU_OK or LGPU_E_NODEVICE

#define LGPU_HIP(expr)                                                              \
  do {                                                                              \
    hipError_t e_ = (expr);                                                         \
    if (e_ != hipSuccess) {                                                         \
      lgpu::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return LGPU_E_HIP;                                                            \
    }                                                                               \
  } while (0)

#define LGPU_REQUIRE(cond, msg)                                   \
  do {                                                            \
    if (!(cond)) { lgpu::set_error("%s: %s", __func__, msg); return LGPU_E_BADARG; } \
  } while (0)

#define LGPU_CHECK_LAUNCH()                                                         \
  do {                                                                              \
    hipError_t e_ = hipGetLastError();                                              \
    if (e_ != hipSuccess) {                                                         \
      lgpu::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
      return LGPU_E_HIP;                                                            \
    }                                                                               \
  } while (0)

// 256-byte LUT passed by value as a kernel argument (lands in the kernarg segment -> scalar loads)
struct Lut8 {
  uint32_t w[64];
};
static inline Lut8 pack_lut(const uint8_t *lut8) {
  Lut8 l;
  if (lut8) __builtin_memcpy(l.w, lut8, 256);
  else for (int i = 0; i < 64; i++) { uint32_t b = 4u * i; l.w[i] = b | ((b + 1) << 8) | ((b + 2) << 16) | ((b + 3) << 24); }
  return l;
}

// The frames of one batched effect launch (lgpu_fx_batch): planes of the first input, of the second input (transitions) and of the output of every frame; the
// kernels take the frame from the grid (z index, or y where the grid is one-dimensional).  A single-frame entry point passes a table with one frame.
struct FxFrames {
  const uint8_t *in0[LGPU_FX_MAX_FRAMES][4];
  const uint8_t *in1[LGPU_FX_MAX_FRAMES][4];
  uint8_t *out[LGPU_FX_MAX_FRAMES][4];
};
// the batched forms behind the single-frame entry points and lgpu_fx_batch (argument checks included; ensure_init() is the caller's)
int softlight_n(const FxFrames &F, int nframes, const int irow[4], const int orow[4], int width, int height, int palette, int unclamped, hipStream_t st);
int blend_chroma_n(const FxFrames &X, int nframes, int irow1, int irow2, int orow, int width, int height, int psize, const int *bf, hipStream_t st);
int blend_luma_n(const FxFrames &X, int nframes, int type, int irow1, int irow2, int orow, int width, int height, int psize, int pal_order, const int *thresh, hipStream_t st);
int blend_multi_n(const FxFrames &X, int nframes, int type, int irow1, int irow2, int orow, int width, int height, int is_bgr, const int *bf, hipStream_t st);
int transition_n(const FxFrames &F, int nframes, int type, int irow1, int irow2, int orow, int width, int height, int psize, const double *amounts, hipStream_t st);
// the geometric transitions (multi_transitions.c:129-150): what the frame's size decides (TransGeom) and what the transition amount decides on top of it (TransAmt),
// derived on the host by the reference's own float / double mix (effects.hip).  lgpu_transition / lgpu_fx_batch and the select form of the one-launch tick
// (flat_select.hip) both call these, so one amount gives one figure.  irow1 is read for type 2 (4 way split) only
struct TransGeom { int wb, ihwidth, ihheight; float hwidth, hheight, maxradsq; };      // wb: bytes of a row (width * psize)
struct TransAmt { int xx, yy; float bf, uthr; };      // type 0: rectangle insets (bytes, rows); type 1: uthr, the largest float u with sqrt((double)(u / maxradsq)) <= bf
TransGeom transition_geometry(int type, int width, int height, int psize);
TransAmt transition_amount(const TransGeom &g, int type, int psize, int irow1, double amount);
int gauss5_colorkey_n(const FxFrames &F, int nframes, int irow0, int irow1, int orow, int width, int height, int psize, int is_bgr, double delta, double opac,
                      int col_r, int col_g, int col_b, hipStream_t st);
int yuv411_to_rgb_n(const FxFrames &F, int nframes, int width_mp, int height, int orow, int out_order, int out_alpha, int clamping_unclamped, hipStream_t st);

// conversion tables resident in device memory (uploaded once by lgpu_init)
struct DeviceTables {
  int32_t *yuv2rgb[4];   // [5][256] each
  int32_t *rgb2yuv[4];   // [9][256] each
  int32_t *luma;         // [3][256]: 65536-scaled unclamped BT.601 luma weights (libweed/weed-plugin-utils.c:879-895)
};
const DeviceTables *device_tables();
int device_cus();      // CUs of the current device

constexpr int kBlock = 256;   // 4 wavefronts of 64

// frames of one geometry for the batch forms of the single-plane kernels (lgpu_*_batch): the frame is the grid's z index; travels in the kernarg segment
struct FrameTab { const uint8_t *src[16]; uint8_t *dst[16]; };        // 16 = LGPU_FX_MAX_FRAMES

// ---- launch-shape switches ------------------------------------------------------------------
// Every switch the launch paths consult lives in ONE process-wide table of atomics: filled once from the environment (LGPU_<NAME>) at first use, changed
// afterwards only through lgpu_tuning_set() (tests, sweeps).  No launch path calls getenv(): the host (LiVES) calls setenv() at run time from other threads.
#define LGPU_TUNE_SWITCHES(X)                                                                                     \
  X(PBH_ALIGNED) X(PBH_TH) X(PBH_ORDER) X(PBH_GROUP) X(PBH_OCC) X(PB_NO_PAIRS) X(PB_UP_RB) X(PB_CACHE_MAX) X(PB_CHAIN_GROUP) \
  X(CHAIN_SPARE_WGS) X(SEP2P_FORCE) X(SOFT_NO_S) X(SOFT_RB) X(EDGE_NO_S) X(EDGE_TH) X(SEAM_STAGED)
enum Tune {
#define LGPU_TUNE_ENUM(n) TUNE_##n,
  LGPU_TUNE_SWITCHES(LGPU_TUNE_ENUM)
#undef LGPU_TUNE_ENUM
  TUNE_COUNT
};
int tune(Tune t);                                  // the value, or -1 when the switch is unset
static inline bool tune_on(Tune t) { return tune(t) > 0; }

static inline unsigned cdiv(unsigned a, unsigned b) { return (a + b - 1) / b; }

// ---- argument checks of the tick's one-launch forms (pixbuf.hip, flat.hip) ------------------------------
// What lgpu_chain_yuv420p, lgpu_chain_to_yuv, lgpu_chain_yuv420p_to_yuv and the lgpu_chain_flat_* forms say about a decoded YUV source, a YUV sink, an RGBA
// destination and a track's pointers is said ONCE, here (defined in pixbuf.hip beside get_sink_tables).  fn: the entry point's name, for set_error.  Each returns
// LGPU_OK or LGPU_E_BADARG, launches and allocates nothing, and is called before the entry point's own LGPU_E_UNSUPPORTED refusals.
// A decoded source of pr->sw x pr->sh: sfmt 4 planar 4:2:0, 5 planar 4:2:2, 2 UYVY, 3 YUYV (a packed frame: istrides[0] alone is read)
int check_yuv_source(const char *fn, const lgpu_chain_params *pr, const lgpu_yuv_source *s, int sfmt);
// A YUV sink of pr->dw x pr->dh.  chain_order: the byte order of the chain's result where the source states it (src->out_order ^ params->swap_rb), which
// sink->in_order must repeat; -1 behind an RGBA source, whose order is the caller's word.  l2rgba: layer 2 is an RGBA frame of rowstride pr->irow2
int check_yuv_sink(const char *fn, const lgpu_chain_params *pr, const lgpu_chain_sink *sk, int chain_order, bool l2rgba);
// An RGBA destination of rowstride pr->orow: the pr->dw x pr->dh frame itself, or the canvas it is letterboxed onto (cv may be null)
int check_rgba_dest(const char *fn, const lgpu_chain_params *pr, const lgpu_canvas *cv, bool l2rgba);
// One track.  src: its source planes, the first nsrc of them required (the others may be null); rgba_src: src[0] is an RGBA frame.  l2: the RGBA layer 2 where one
// is read (l2rgba).  dst: ndst destination planes, none of them a source plane; rgba_dst: dst[0] is an RGBA frame
int check_track(const char *fn, const uint8_t *const src[3], int nsrc, bool rgba_src, const uint8_t *l2, bool l2rgba, uint8_t *const *dst, int ndst, bool rgba_dst);
// The kernels address a plane through 32-bit offsets: LGPU_E_UNSUPPORTED when one of `bytes` (rows x rowstride, or a plane's size) is 2 GiB or more.  instead: what
// to run then, for the message
int check_plane_sizes(const char *fn, std::initializer_list<long long> bytes, const char *instead = nullptr);

#if defined(__HIPCC__)
// ---- device helpers ---------------------------------------------------------------------------------
// stage a kernarg LUT into LDS (256 B) -- one dword per lane for the first wave
__device__ __forceinline__ void stage_lut(uint8_t *lds_lut, const Lut8 &lut) {
  if (threadIdx.x < 64) reinterpret_cast<uint32_t *>(lds_lut)[threadIdx.x] = lut.w[threadIdx.x];
}
__device__ __forceinline__ uint32_t lut3_rgba(const uint8_t *l, uint32_t p) {   // LUT on bytes 0..2, keep byte 3
  return (uint32_t)l[p & 0xFF] | ((uint32_t)l[(p >> 8) & 0xFF] << 8) | ((uint32_t)l[(p >> 16) & 0xFF] << 16) | (p & 0xFF000000u);
}
__device__ __forceinline__ uint32_t lut3_argb(const uint8_t *l, uint32_t p) {   // LUT on bytes 1..3, keep byte 0
  return (p & 0xFFu) | ((uint32_t)l[(p >> 8) & 0xFF] << 8) | ((uint32_t)l[(p >> 16) & 0xFF] << 16) | ((uint32_t)l[p >> 24] << 24);
}
__device__ __forceinline__ uint32_t lut4(const uint8_t *l, uint32_t p) {
  return (uint32_t)l[p & 0xFF] | ((uint32_t)l[(p >> 8) & 0xFF] << 8) | ((uint32_t)l[(p >> 16) & 0xFF] << 16) | ((uint32_t)l[p >> 24] << 24);
}
__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
// K2's per-pixel arithmetic on its paired tables (src/colourspace.c:3445-3554, xyuv2rgb :2351-2356), shared by the converter (yuv.hip, k_yuv420p_to_rgb_s) and the
// 2:1 chain with a 4:2:0 source (pixbuf.hip, k_pb_half<.., YUV>) so that the two cannot drift apart.  Chroma (2a + b) / 3 on doubled sums:
// (int)(s / 3. + .5) == (s + 1) / 3 == (s + 1) * 43691 >> 17 for s < 2^15
__device__ __forceinline__ uint32_t yuv_third(uint32_t s1, uint32_t s2) { return __umul24(s1 + (s2 >> 1) + 1u, 43691u) >> 17; }
// RGB_Y[y] + {R_Cr, G_Cr}[v] + {G_Cb, B_Cb}[u], >> 16, CLAMP0255
__device__ __forceinline__ void yuv_rgb(uint32_t yy, uint32_t rcr, uint32_t gcr, uint32_t gcb, uint32_t bcb, uint32_t &r, uint32_t &g, uint32_t &b) {
  const int sr = (int)(yy + rcr), sg = (int)(yy + gcb + gcr), sb = (int)(yy + bcb);
  r = (uint32_t)min(max(sr >> 16, 0), 255); g = (uint32_t)min(max(sg >> 16, 0), 255); b = (uint32_t)min(max(sb >> 16, 0), 255);
}
// init_average's clamped chroma average (src/colourspace.c:190-216; palette.hip has the table form, cavg_lds, and compares the two over all 65,536 pairs when the
// table is built: cavg_forms_checked()).
// fa(x) WITHOUT the table: d = x - 128 is exact in float, 255 / 244 = KHI + KLO to 48 bits, and fmaf(d, KHI, d * KLO) rounds the exact d * KHI + fl(d * KLO) once --
// for all 256 bytes the float the double division gives (k_build_cavgc compares the two forms entry by entry; tests/test_gpu_parity.py::test_chroma_average_table).
// Four vector operations instead of an LDS gather: for kernels whose LDS pipe is full of table gathers (YUV411 -> RGB: 67 % bank-conflict cycles).
__device__ __forceinline__ float cavg_fa_arith(float d) { return __fmaf_rn(d, 0x1.0b8a7ep+0f, __fmul_rn(d, -0x1.92e2ap-28f)); }
__device__ __forceinline__ int cavg_arith(int clamped, int x, int y) {
  if (!clamped) {
    const int c = (((x - 128) + (y - 128)) >> 1) + 128;
    return c > 255 ? 255 : c < 0 ? 0 : c;
  }
  const float fc = __fmaf_rn(__fadd_rn(cavg_fa_arith((float)(x - 128)), cavg_fa_arith((float)(y - 128))), 0.4375f, 128.f);
  return (int)__builtin_amdgcn_fmed3f(fc, 16.f, 240.f);
}
// chroma blend of simple_blend.c:117-146 on an RGBA pair (the staged path's form): opaque layer-2 pixels through the integer table expression, translucent ones
// through the reference's float scaling of both sources first; dst alpha = the track's alpha
__device__ __forceinline__ uint32_t pb_chroma_rgba(uint32_t p1, uint32_t p2, uint32_t bf, uint32_t nbf) {
  const uint32_t al = p2 >> 24;
  uint32_t s1 = p1, s2 = p2;
  if (al != 255) {
    const float alpha = (float)((double)(float)al / 255.), inv = (float)(1. - (double)alpha);
    s1 = 0; s2 = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      s2 |= ((uint32_t)(int)__fmul_rn((float)((p2 >> (8 * c)) & 0xFF), alpha) & 0xFF) << (8 * c);
      s1 |= ((uint32_t)(int)__fmul_rn((float)((p1 >> (8 * c)) & 0xFF), inv) & 0xFF) << (8 * c);
    }
  }
  const uint32_t lo = ((__umul24(s2 & 0x00FF00FFu, bf) + __umul24(s1 & 0x00FF00FFu, nbf)) >> 8) & 0x00FF00FFu;
  const uint32_t hi = ((__umul24((s2 >> 8) & 0xFFu, bf) + __umul24((s1 >> 8) & 0xFFu, nbf))) & 0x0000FF00u;
  return lo | hi | (p1 & 0xFF000000u);
}
// the same blend where layer 2 is opaque by construction (a frame K2 has just converted: alpha 255): the integer expression alone, no float path to instantiate
__device__ __forceinline__ uint32_t pb_chroma_opaque(uint32_t p1, uint32_t p2, uint32_t bf, uint32_t nbf) {
  const uint32_t lo = ((__umul24(p2 & 0x00FF00FFu, bf) + __umul24(p1 & 0x00FF00FFu, nbf)) >> 8) & 0x00FF00FFu;
  const uint32_t hi = ((__umul24((p2 >> 8) & 0xFFu, bf) + __umul24((p1 >> 8) & 0xFFu, nbf))) & 0x0000FF00u;
  return lo | hi | (p1 & 0xFF000000u);
}
// [1 4 6 4 1] on packed 16-bit lanes, a + e + 4 (b + d) + 6 c + k, without a 32-bit multiply: the operands of the vertical pass exceed 24 bits, so `6u * c` became
// v_mul_lo_u32 (a quarter of the vector rate); ((b + c + d) << 2) + (c << 1) + (a + e + k) is two v_add3 and two v_lshl_add
__device__ __forceinline__ uint32_t gauss5_taps(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t e, uint32_t k = 0u) { return ((b + c + d) << 2) + (c << 1) + (a + e + k); }

// --- per-lane 4-pixel gather / scatter ------------------------------------------------------------------
// 3-byte pixels: 12 contiguous bytes d0 d1 d2 -> four dwords [c0 c1 c2 x]
__device__ __forceinline__ void unpack3(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t p[4]) {
  p[0] = d0;
  p[1] = __builtin_amdgcn_perm(d1, d0, 0x0C050403u);   // d0.b3 d1.b0 d1.b1
  p[2] = __builtin_amdgcn_perm(d2, d1, 0x0C040302u);   // d1.b2 d1.b3 d2.b0
  p[3] = d2 >> 8;
}
// four dwords [o0 o1 o2 x] -> 12 contiguous bytes
__device__ __forceinline__ void pack3(const uint32_t q[4], uint32_t &w0, uint32_t &w1, uint32_t &w2) {
  w0 = __builtin_amdgcn_perm(q[1], q[0], 0x04020100u);   // q0.b0 q0.b1 q0.b2 q1.b0
  w1 = __builtin_amdgcn_perm(q[2], q[1], 0x05040201u);   // q1.b1 q1.b2 q2.b0 q2.b1
  w2 = __builtin_amdgcn_perm(q[3], q[2], 0x06050402u);   // q2.b2 q3.b0 q3.b1 q3.b2
}

#endif

}  // namespace lgpu
