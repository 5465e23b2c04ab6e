/* lives_gpu_select.h -- select transitions between two decoded clips in ONE launch (liblivesgpu.so, gfx950).

   lives_gpu.h's lgpu_chain_flat_yuv_mix[_canvas] mix two decoded frames with the chroma blend, which needs both layers at every pixel.  The transitions a LiVES set
   uses between clips -- "iris rectangle", "iris circle" and "dissolve" of multi_transitions.c -- SELECT: a pixel shows layer 1 or layer 2, and which one is known from
   its coordinates, the amount and (dissolve) the mask before anything is loaded.  The entry point below decides first and converts only the layer a pixel shows: a wave
   wholly inside or wholly outside the figure loads and converts ONE layer, and at amount 0 or 1 -- the two ends of every transition -- every wave does. */
#ifndef LIVES_GPU_SELECT_H
#define LIVES_GPU_SELECT_H

#include "lives_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the transition: multi_transitions.c's `type` numbers */
#define LGPU_SELECT_IRIS_RECT   0
#define LGPU_SELECT_IRIS_CIRCLE 1
#define LGPU_SELECT_DISSOLVE    3
typedef struct { int kind;                   /* 0 iris rectangle, 1 iris circle, 3 dissolve */
                 const double *amounts;      /* ntracks transition amounts, 0..1 (host memory): 0 shows layer 1 everywhere, 1 layer 2 (the reference's circle tests
                                                radius > amount, so a pixel at the figure's very centre, radius 0, is layer 2's at amount 0 too) */
                 const float *const *mask_d; /* dissolve: ntracks DEVICE pointers (a host table of them), each to (canvas or frame) width * height floats as
                                                lgpu_dissolve_mask lays them out; not read otherwise and may be NULL */
               } lgpu_select;

/* lgpu_chain_flat_yuv_select: two decoded frames, each YUV420P, YUV422P, UYVY or YUYV under its own lgpu_yuv_layer_source and both sw x sh, through a select transition,
   [the gamma LUT] and to RGBA or a YUV sink, as ONE launch with no RGBA frame anywhere.  Sources, tracks, sink and canvas are exactly what lgpu_chain_flat_yuv_mix and
   lgpu_chain_flat_yuv_mix_canvas accept: lgpu_chain_yuv_mix_track (a packed layer is its y_d / y2_d with rowstride istrides[0]; its chroma pointers are not read and
   may be NULL), src2->out_order == src->out_order ^ params->swap_rb, LGPU_INTERP_PIXBUF required, sw == dw and sh == dh, no sink behind a canvas, the mix form's
   alignment rules.  params->bf, params->irow2 and LGPU_INTERP_NOBLEND are not read.

   The bytes are DEFINED, per track and bit for bit, as those of this sequence:
     1. layer 2 through the single-frame call of src2->in_fmt into a tight sw x sh RGBA frame B, as lgpu_chain_flat_yuv_mix defines it (lgpu_yuv420p_to_rgb with
        is_422 0 / 1, or lgpu_yuv_to_rgb; opsize 4, src2->out_order, src2's tables, pb_quality and flags, no LUT);
     2. layer 1 the same way under src into A, then R <-> B (lgpu_swizzle, swap3postalpha) if params->swap_rb;
     3. with a canvas, lgpu_letterbox_at(.., sw, sh, .., nwidth, nheight, 4, {0, 0, 0, 255}, offs_x, offs_y) on both, onto opaque black;
     4. lgpu_transition(kind, A, B, .., psize 4, amount) for kinds 0 and 1, lgpu_dissolve(A, B, .., psize 4, mask_d[track], amount) for kind 3, at the canvas's size, or
        the frame's without a canvas: the figure is the canvas's, its insets in bytes of 4-byte pixels, and the mask is indexed by canvas row * nwidth + canvas column;
     5. lgpu_gamma_apply with params->lut8 if params->use_lut (a bar pixel is select(black, black) = opaque black, then the LUT; nothing is read for it);
     6. with a sink, lgpu_rgb_to_yuv(.., sink->in_order, 1, .., sink->out_fmt, 0, sink->which_tables), every K4 quirk kept: the 4:2:0 chroma of a row pair comes from
        whichever layers' pixels the pair shows.
   Without a sink the result is RGBA in dst_d[0] with rowstride params->orow, canvas-sized with a canvas.

   LGPU_E_BADARG: what lgpu_chain_flat_yuv_mix[_canvas] call a bad argument (LGPU_INTERP_NOBLEND and the uint8 amounts apart); a canvas together with a sink; a kind
   other than 0, 1 or 3; null sel or sel->amounts; an amount outside 0..1 or not finite; dissolve with a null mask table or a null mask pointer; a mask address that is
   not a multiple of 4.  LGPU_E_UNSUPPORTED: what lgpu_chain_flat_yuv_mix[_canvas] refuse.  Everything is checked before anything is allocated or enqueued: a refused
   call writes nothing.

   Stream contract: the amounts' four derived values and the mask pointers travel in the kernel's arguments, LGPU_CHAIN_SELECT_TRACKS tracks per launch, 33..64 tracks as
   two launches on `stream`.  A warm call allocates nothing and waits for nothing, so it can be captured into a graph (the host arrays are read during the call; the
   mask POINTERS are baked into a captured launch, the masks' contents are read at replay).  With a sink, the first call with a new (sink->which_tables, sink->in_order)
   pair builds a device table with a blocking allocation and copy outside `stream`, as in lgpu_chain_to_yuv; to YUV420P the first call of the process also checks the
   chroma-average forms once.  Nothing else is uploaded: the K2 tables are lgpu_init's.

   Out of scope, each for its reason: "4 way split" and "slide over" show layer 1 at a SHIFTED position, and K2's walk depends on the position (the seeded first pair of a
   row, the chroma rows a row pair reads), so a shifted pixel is not the cell's own conversion; "rand replace" keeps state from frame to frame; the luma overlays decide
   by ONE layer's luma, a predicate that comes from data and not from coordinates: they are lives_gpu_luma.h's lgpu_chain_flat_yuv_luma.  Recording a transition class as a deferred stage of the layer seam
   (lives_gpu_layer.h) is a follow-up; livesgpu_fx.so keeps its classes and its process functions. */
#define LGPU_CHAIN_SELECT_TRACKS 32   /* tracks per launch of lgpu_chain_flat_yuv_select */
int lgpu_chain_flat_yuv_select(const lgpu_chain_params *params, const lgpu_yuv_layer_source *src, const lgpu_yuv_layer_source *src2, const lgpu_select *sel,
                               const lgpu_canvas *canvas /* NULL or RGBA only */, const lgpu_chain_sink *sink /* NULL: RGBA into dst_d[0], rowstride params->orow */,
                               const lgpu_chain_yuv_mix_track *tracks, int ntracks, void *stream);

#ifdef __cplusplus
}
#endif
#endif
