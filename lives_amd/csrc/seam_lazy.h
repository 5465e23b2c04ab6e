// seam_lazy.h -- deferred programs on pinned layers (definitions: seam_lazy.cpp): the stages a program can take, the program itself (struct Lazy), what the seam
// bodies call to record a stage (lazy_detach, lazy_attach / lazy_reattach, lazy_commit, lazy_record_yuv) and the three hooks of the residency unit.
#pragma once
#include <atomic>
#include "seam_resident.h"

#pragma GCC visibility push(hidden)
namespace seam {

// ---- deferred execution on pinned layers ------------------------------------------------------------------------------------------------
// The host bytes of a pinned layer are stale by contract until lives_gpu_layer_sync(), so nothing obliges a seam call on a pinned layer to have RUN when it
// returns -- only to have happened, in order, before anybody sees the pixels.  The calls of one track's plan step (src/nodemodel.c:1065-1253: pconv, resize,
// letterbox substeps; src/effects-weed.c:1850-2425: the filter instance; the gamma substep) on an RGBA32 / BGRA32 frame are therefore RECORDED on the plane
// instead of launched one by one: R <-> B swizzle, gdk-pixbuf scale, letterbox canvas, "chroma blend" with a second layer, gamma LUT -- in that order, each at
// most once.  Every leaf of the layer changes exactly as in the eager call (palette, size, rowstrides, a fresh host plane, gamma tag); the plane's entry in the
// residency table holds the program instead of pixels.  A program runs
//   * when someone needs the pixels (any other seam call or effect on the plane, lives_gpu_layer_sync / _unpin: through acquire()), by itself;
//   * when lives_gpu_layers_flush() is handed the layers of a tick: programs of equal shape become ONE launch of the fused chain kernel (lgpu_chain /
//     lgpu_chain_canvas, one track per layer) -- the launch bench.py times, reached through the reference's own calls;
//   * before a plane it reads (layer 2 of its blend) is written, replaced or released.
// What a stage could refuse is checked when it is recorded (palette, geometry, the scaler's range), so a recorded call cannot turn into a FALSE later; a device
// failure at run time (allocation, launch) surfaces at the flush / sync that runs the program, which then stays pending.
// lives_gpu_set_deferred(0) switches the recording off (every call launches its own kernels, as before round 6); tests compare the two.
// LZ_YUV: a decoder's YUV420P / YVU420P frame converted to RGBA32 / BGRA32 (K2, no gamma change) -- the program then owns (or, for surfaces of
// lives_gpu_layer_pin_device, borrows) the three source planes and stands for the new RGBA host plane; the stages above are recorded on top of it.
// LZ_SINK: the RGBA32 / BGRA32 frame converted to the consumer's YUV palette (K4: YUV420P / YVU420P / UYVY / YUYV, no gamma change) -- the last stage a program
// can take.  The program then stands for up to THREE host planes: each has its own table entry pointing at the one Lazy (sph: the planes in the conversion's
// Y, U, V order), so a read, sync or seam call on ANY of them runs it, and whichever entry is dropped first takes the others with it (lazy_discard).
enum { LZ_NONE = 0, LZ_YUV = 1, LZ_SWAP = 2, LZ_SCALE = 3, LZ_CANVAS = 4, LZ_BLEND = 5, LZ_LUT = 6, LZ_SINK = 7 };
struct Lazy {
  Dev src;                          // the frame the program starts from (owned: goes back to the pool when the program has run, unless external)
  int sw = 0, sh = 0, srs = 0;
  int stage = LZ_NONE;              // the last stage recorded
  bool swap = false;
  bool scale = false; int dw = 0, dh = 0, interp = 0; bool opaque = false;     // opaque: the layer carried the host's word when the scale was recorded
  bool canvas = false; int nw = 0, nh = 0, ox = 0, oy = 0;
  bool blend = false; int bf = 0; const void *l2h = nullptr; Dev l2; int l2rs = 0;
  // lives_gpu_set_pending_layer2: layer 2 was itself a pending program when the blend was recorded and was NOT run for it -- l2 is empty, l2h names its plane (whose
  // lazy_readers counts this program as for a resident plane).  Whoever runs this program looks at that entry first (g_lazy_mu held): still a program -- it is folded
  // into the launch or run ahead of it; pixels meanwhile -- they become l2 and the flag goes
  bool l2pend = false;
  bool lut = false; uint8_t lut8[256];
  int w = 0, h = 0, rs = 0;         // the plane the program stands for
  // LZ_YUV: src is the luma plane; yu / yv the chroma planes (U, V order: a YVU420P layer's planes are swapped when recorded).  yfmt: the source's format in
  // lgpu_rgb_to_yuv's numbers -- 4 planar 4:2:0, 5 YUV422P, 2 UYVY, 3 YUYV (src is the one packed plane, yu / yv are empty, ystr[0] its rowstride).  The 2:1 and
  // 4:2:0 flat chains (lgpu_chain_yuv420p[_to_yuv], lgpu_chain_flat_yuv420p*) take yfmt 4 ONLY: every read of `yuv` that leads to one of them tests it
  bool yuv = false; int yfmt = 4; Dev yu, yv; int ystr[3] = {0, 0, 0}; long usz = 0, vsz = 0; int order = 0, which = 0, quality = 2;
  // LZ_SINK: K4 on the w x h RGBA plane above (sww x shh of it: 4:2:0 truncates to even sides) into snp planes of sors / sbytes, registered under host planes sph
  bool sink = false; int sfmt = 0, swhich = 0, sorder = 0, snp = 0, sww = 0, shh = 0, sors[3] = {0, 0, 0}; size_t sbytes[3] = {0, 0, 0}; const void *sph[3] = {nullptr, nullptr, nullptr};
};
extern std::atomic<unsigned long long> g_lz_recorded, g_lz_sink_recorded;      // lives_gpu_deferred_stats_n [0], [8]: the seam body that records LZ_SINK counts its own
inline bool lazy_pal(int pal) { return pal == WEED_PALETTE_RGBA32 || pal == WEED_PALETTE_BGRA32; }

// the residency unit's hooks: a pending program nobody will look at goes; programs that read plane h run before h changes; the program of plane h runs now
void lazy_discard(Lazy *z);
void lazy_run_readers_of(const void *h);
bool lazy_materialise(const void *h);

Lazy *lazy_detach(const Layer &l, int stage);
void lazy_attach(const void *h, Lazy *z);
void lazy_reattach(const void *h, Lazy *z);
bool lazy_commit(weed_plant_t *layer, const Layer &l, Lazy *z, int pal, int width, int height, int alignment);
bool lazy_record_yuv(weed_plant_t *layer, const Layer &l, int outpl, int which, int new_gamma, int flags);

}  // namespace seam
#pragma GCC visibility pop
