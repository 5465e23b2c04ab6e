/* lives_gpu_luma.h -- luma overlays between two decoded clips in ONE launch (liblivesgpu.so, gfx950).

   The four luma classes of simple_blend.c:151-194 -- "luma overlay", "luma underlay", "negative luma overlay" and "averaged luma overlay" (which is the overlay in the
   reference: its 3x3 branch is never reached) -- SELECT like the transitions of lives_gpu_select.h: a pixel shows layer 1 or layer 2.  Which one is decided by ONE
   layer's luma, the KEYED layer's: layer 1's for types 1, 3 and 4, layer 2's for type 2.  The other layer is needed only where it is shown.  The entry point below
   converts the keyed layer, decides per pixel, and loads and converts the other layer only in waves that show some of it: at threshold 0 no wave does. */
#ifndef LIVES_GPU_LUMA_H
#define LIVES_GPU_LUMA_H

#include "lives_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { int type;                  /* 1 overlay, 2 underlay, 3 negative overlay, 4 averaged (== 1) */
                 const uint8_t *thresholds; /* ntracks values 0..255, host memory */ } lgpu_luma_key;

/* lgpu_chain_flat_yuv_luma: two decoded frames, each YUV420P, YUV422P, UYVY or YUYV under its own lgpu_yuv_layer_source and both sw x sh, through a luma overlay,
   [the gamma LUT] and to RGBA or a YUV sink, as ONE launch with no RGBA frame anywhere.  Sources, tracks, canvas, sink, alignment rules and refusals are exactly those
   of lgpu_chain_flat_yuv_select (lives_gpu_select.h): src2->out_order == src->out_order ^ params->swap_rb, LGPU_INTERP_PIXBUF required, sw == dw and sh == dh, a canvas
   with RGBA only, 1..64 tracks.  params->bf, params->irow2 and LGPU_INTERP_NOBLEND are not read.

   The bytes are DEFINED, per track and bit for bit, as lives_gpu_select.h's six steps with step 4 replaced by
     4. lgpu_blend_luma(key->type, A, .., B, .., dst = A, .., psize 4, pal_order = src->out_order ^ params->swap_rb, key->thresholds[track]) at the canvas's size, or the
        frame's without a canvas.  It runs in place on A, so byte 3 stays A's 255: type 1 / 4 shows B where luma(A) < threshold, type 3 where luma(A) > 255 - threshold,
        type 2 where luma(B) > 255 - threshold.  Threshold 0 shows layer 1 everywhere, for every type.
   A bar pixel of the canvas is a choice between black and black, then the LUT; nothing is read for it.

   LGPU_E_BADARG: what lgpu_chain_flat_yuv_select calls a bad argument (its own kind, amounts and masks apart); null key or key->thresholds; a type outside 1..4.
   LGPU_E_UNSUPPORTED: what lgpu_chain_flat_yuv_select refuses.  Everything is checked before anything is allocated or enqueued: a refused call writes nothing.

   Stream contract: lgpu_chain_flat_yuv_select's.  The thresholds travel in the kernel's arguments, LGPU_CHAIN_LUMA_TRACKS tracks per launch, 33..64 tracks as two
   launches on `stream`.  A warm call allocates nothing and waits for nothing, so it can be captured into a graph (the host array is read during the call).  With a sink,
   the first call with a new (sink->which_tables, sink->in_order) pair builds a device table outside `stream`, as in lgpu_chain_to_yuv.

   Out of scope: recording the class as a deferred stage of the layer seam (lives_gpu_layer.h); livesgpu_fx.so's process functions; multi_blends.c, which is RGB24-only
   in the reference. */
#define LGPU_CHAIN_LUMA_TRACKS 32   /* tracks per launch of lgpu_chain_flat_yuv_luma */
int lgpu_chain_flat_yuv_luma(const lgpu_chain_params *params, const lgpu_yuv_layer_source *src, const lgpu_yuv_layer_source *src2,
                             const lgpu_luma_key *key, const lgpu_canvas *canvas /* NULL or RGBA only */, const lgpu_chain_sink *sink /* NULL: RGBA into dst_d[0] */,
                             const lgpu_chain_yuv_mix_track *tracks, int ntracks, void *stream);

#ifdef __cplusplus
}
#endif
#endif
