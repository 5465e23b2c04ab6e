// flat_plan.h -- the host side that every lgpu_chain_flat_* entry point shares (flat.hip's blend and mix forms, flat_select.hip's select form), said ONCE and defined
// in flat.hip as the check_* functions of lgpu_common.h are defined in pixbuf.hip: the description of a decoded layer, the track record, the refusal sequence with
// the plan it returns, the launch shape, and the way from run-time values to template arguments.  A new form is a kernel, one fill function per argument struct and
// a few lines that call these.
#pragma once
#include "lgpu_common.h"
#include <type_traits>

#pragma GCC visibility push(hidden)      // internal to the library: the exported names stay the public headers' and what they were
namespace lgpu {

// One decoded layer.  ys: the source as the shared checks read it (check_yuv_source); what a packed layer does not have -- chroma rowstrides and plane sizes -- is
// zeroed by flat_layer and nowhere else.  The rest is the kernels' view of it
struct FlatLayer {
  lgpu_yuv_source ys;
  int fmt;                       // 2 UYVY, 3 YUYV, 4 YUV420P, 5 YUV422P
  bool packed;
  int policy;                    // the kernels' source policy (SRC; L2YUV - 1; SRC2): 0 planar 4:2:0, 1 planar 4:2:2, 2 packed 4:2:2
  const int32_t *tables;         // device [5][256] of ys.which_tables
  int clamped;                   // the 16..240 chroma clamp folded into the staged tables' index: K3 indexes its tables with the sample itself
  int lowq, fix_edges;
  int sfmt;                      // packed: fmt; 0 otherwise
};
// after ensure_init(); an in_fmt is the caller's to check first
FlatLayer flat_layer(const lgpu_yuv_source *s);            // planar 4:2:0
FlatLayer flat_layer(const lgpu_yuv422_source *s);
FlatLayer flat_layer(const lgpu_yuv_layer_source *s);
// one staged copy of the K2 tables serves both layers when they index the same set the same way.  A planar layer with clamped tables indexes rg / gb through the
// 16..240 clamp that staging folds into the index, a packed layer with the sample itself: UYVY over YUV420P, both with which_tables 0, needs two copies
static inline bool flat_tables_shared(const FlatLayer &a, const FlatLayer &b) { return a.tables == b.tables && a.clamped == b.clamped; }

// One track of any entry point: layer 1's planes, the RGBA layer 2 (the blend forms), a decoded layer 2's planes (the mix and select forms), the destination's.
// Each entry point fills an array of these from its own public track type, once; the checks and the per-launch fills read nothing else
struct FlatTrack {
  const uint8_t *y, *u, *v, *l2, *y2, *u2, *v2;
  uint8_t *dst[3];
};
// from the mix and select forms' tracks.  packed1: layer 1 is its y plane alone -- its chroma pointers are not read, so they may be null and are no plane a
// destination could collide with
void flat_tracks(FlatTrack *out, const lgpu_chain_yuv_mix_track *tracks, int ntracks, bool packed1);

struct FlatPlan {
  int chain_order;               // the byte order the chain works in: src->out_order ^ params->swap_rb
  bool planar;                   // the 4:2:0 sink
  int nplanes, sink;             // destination planes; the kernels' SINK: 0 RGBA, 1 packed 4:2:2, 2 planar 4:2:0
  bool noblend, l2rgba;          // LGPU_INTERP_NOBLEND where it means something; layer 2 is an RGBA frame of rowstride irow2
  int w, h;                      // the frame
  int drow, irow2, urow, vrow;   // destination (RGBA / packed / luma), RGBA layer 2 and 4:2:0 chroma rowstrides
  int fw, fh;                    // the destination's frame: the canvas, or the frame without one
  int cw, ch, ox, oy;            // canvas (cw == 0: none)
  int fmt, unclamped, use_lut;   // sink: 2 UYVY, 3 YUYV, 4 YUV420P
  int hw, nunits;                // chroma columns; units of K2's walk (row 0, the row pairs, the trailing row of an even height)
  unsigned gx;
  long long bar_px;              // pixels of the canvas's bars
  const uint2 *stab;             // sink: device [2][3][256] (get_sink_tables)
  Lut8 lut;
};
// THE refusal sequence of the unscaled tick: the gdk-pixbuf arithmetic, [NOBLEND, amounts,] check_yuv_source per layer, layer 2's byte order, sink or RGBA destination,
// each track (check_track, layer 2's null planes, plane / destination collisions), then LGPU_E_UNSUPPORTED: frames that keep their size (keep_size: the message, with
// the caller's hint of what to run instead), the gaussian, the packed layers' alignment, the sink's refusals, planes of 2 GiB or more; last the sink's tables.  Every
// LGPU_E_BADARG comes before any LGPU_E_UNSUPPORTED and everything before anything is allocated or enqueued.  l2: a decoded layer 2, or null (an RGBA frame per
// track unless LGPU_INTERP_NOBLEND).  select: the select form -- LGPU_INTERP_NOBLEND means nothing there and the amounts are its own; the blend and mix forms
// require amounts unless NOBLEND, which the mix forms refuse
int flat_plan(const char *fn, bool select, const char *keep_size, const lgpu_chain_params *pr, const FlatLayer &l1, const FlatLayer *l2, const lgpu_canvas *cv,
              const lgpu_chain_sink *sk, const FlatTrack *tracks, int ntracks, const uint8_t *amounts, FlatPlan *plan);

// The launch of n tracks: about kFlatWgTarget workgroups, each walking a run of `per` consecutive units on one staging of the tables (blockIdx.y < gy_units), and
// behind them the workgroups that write the canvas's bars
constexpr int kFlatWgTarget = 2048;       // workgroups a launch aims at: each walks nunits * gx * ntracks / 2048 units (at least one) on one staging of the tables
struct FlatShape { int per, gy_units; dim3 grid; };
FlatShape flat_launch_shape(const FlatPlan &p, int n);

// what FlatArgs and SelLayer say about a layer, and FlatArgs and SelArgs about the frame, its destination and the launch: the same fields under the same names
template <class L> static inline void flat_fill_layer(L &d, const FlatLayer &l) {
  d.tables = l.tables; d.usize = (uint32_t)l.ys.u_size; d.vsize = (uint32_t)l.ys.v_size; d.ys = l.ys.istrides[0]; d.us = l.ys.istrides[1]; d.vs = l.ys.istrides[2];
  d.clamped = l.clamped; d.lowq = l.lowq; d.fix_edges = l.fix_edges; d.sfmt = l.sfmt;
}
template <class A> static inline void flat_fill_frame(A &a, const FlatPlan &p) {
  a.stab = p.stab; a.w = p.w; a.h = p.h; a.orow = p.drow; a.urow = p.urow; a.vrow = p.vrow; a.cw = p.cw; a.ch = p.ch; a.ox = p.ox; a.oy = p.oy;
  a.use_lut = p.use_lut; a.fmt = p.fmt; a.unclamped = p.unclamped;
}

// f(std::integral_constant<int, v>()) for a run-time v in 0..N-1 (anything else: 0): the way from run-time values to template arguments, nested where several are
// dispatched.  Every kernel named in f is instantiated for each of the N values
template <int N, class F> static inline void with_constant(int v, F &&f) {
  if constexpr (N > 1) {
    if (v == N - 1) return f(std::integral_constant<int, N - 1>());
    return with_constant<N - 1>(v, f);
  } else f(std::integral_constant<int, 0>());
}

}  // namespace lgpu
#pragma GCC visibility pop
