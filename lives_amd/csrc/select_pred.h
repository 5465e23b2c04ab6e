// select_pred.h -- which of its two layers a pixel of a select transition shows (lives-plugins/weed-plugins/multi_transitions.c:152-212): iris rectangle (type 0),
// iris circle (type 1) and dissolve (type 3).  Stated ONCE: effects.hip's k_transition (trans_from) and k_dissolve, which move RGB(A) pixels, and flat_select.hip's
// k_flat_select, which converts only the layer a pixel shows, take the predicate from here.  What the transition amount decides (xx, yy, bf, uthr: TransAmt) is
// derived on the host by transition_amount (lgpu_common.h, defined in effects.hip) for both.
#pragma once
#include "lgpu_common.h"

namespace lgpu {
#if defined(__HIPCC__)
// The rectangle and the dissolve are EXPRESSIONS (macros), not functions: a `?:` or an `if` on the short-circuit expression itself compiles to the branches k_transition
// and k_dissolve always had, a bool returned from an inlined function does not (tools/isa_compare.py), and those two kernels keep their machine code.
// iris rectangle (:152-160): layer 1 outside the rectangle.  i: the row; j: the BYTE column of the pixel (PS * x); xx: the inset in bytes, yy: in rows; wb: the bytes of
// a row (PS * width)
#define LGPU_IRIS_RECT_SHOWS1(i, j, xx, yy, wb, height) ((j) < (xx) || (j) >= (wb) - (xx) || (i) < (yy) || (i) >= (height) - (yy))
// iris circle (:185-187): sqrt((xxf * xxf + yyf * yyf) / maxradsq) > bf shows layer 1: float terms, double square root.
// The float division by maxradsq and the double square root are monotone in u = xxf^2 + yyf^2, so "sqrt(u / maxradsq) > bf" is "u > uthr" for the one float
// uthr the host finds with the same IEEE operations (exact: every float u falls on the same side); a division and a square root per pixel less
template <int PS>
__device__ __forceinline__ float iris_circle_u(int i, int j, int ihwidth, int ihheight) {
  const float xxf = (float)(i - ihheight), yyf = __fdiv_rn((float)(j - ihwidth), (float)PS);
  return __fadd_rn(__fmul_rn(xxf, xxf), __fmul_rn(yyf, yyf));
}
#define LGPU_IRIS_CIRCLE_SHOWS1(PS, i, j, ihwidth, ihheight, uthr) (lgpu::iris_circle_u<PS>(i, j, ihwidth, ihheight) > (uthr))
// dissolve (:208-212): layer 2 where the pixel's mask value is below the amount.  mask: width * height floats; x: the PIXEL column
#define LGPU_DISSOLVE_SHOWS2(mask, width, i, x, bf) ((mask)[(size_t)(i) * (width) + (x)] < (bf))
#endif
}  // namespace lgpu
