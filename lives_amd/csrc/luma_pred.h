// luma_pred.h -- which of its two layers a pixel of a luma overlay shows (lives-plugins/weed-plugins/simple_blend.c:151-194): overlay (type 1), underlay (2), negative
// overlay (3) and averaged overlay (4, which never reaches its 3x3 branch in the reference and is type 1).  Stated ONCE: effects.hip's LumaBlend, which moves RGB(A)
// pixels, and flat_luma.hip's k_flat_luma, which converts the other layer only where it is shown, take the luma and the comparison from here.  The predicate reads ONE
// layer's luma -- the KEYED layer: layer 2 for type 2, layer 1 otherwise.
#pragma once
#include "lgpu_common.h"

namespace lgpu {
// the layer whose luma decides: 2 for the underlay, 1 for the others
static inline int luma_keyed_layer(int type) { return type == 2 ? 2 : 1; }
#if defined(__HIPCC__)
// luma of a normalised pixel, calc_luma() (libweed/weed-plugin-utils.c:924-934).  s: the [3][256] table of DeviceTables::luma (an LDS copy); order 0 RGB, 1 BGR
__device__ __forceinline__ uint32_t luma_px(const int32_t *s, uint32_t p, int order) {
  const uint32_t c0 = p & 0xFF, c1 = (p >> 8) & 0xFF, c2 = (p >> 16) & 0xFF;
  const int32_t v = order ? (s[c2] + s[256 + c1] + s[512 + c0]) : (s[c0] + s[256 + c1] + s[512 + c2]);
  return (uint32_t)(v >> 16) & 0xFF;
}
// EXPRESSIONS (macros), as select_pred.h's are.  l: the keyed layer's luma; bf: the threshold & 0xFF; neg: 0xFF - bf.  True: the pixel is layer 2's
#define LGPU_LUMA_BELOW(l, bf) ((l) < (bf))       // types 1 and 4 (:151-165): layer 2 where layer 1 is darker than the threshold
#define LGPU_LUMA_ABOVE(l, neg) ((l) > (neg))     // type 2 (:166-179, l is layer 2's) and type 3 (:180-194, l is layer 1's)
#endif
}  // namespace lgpu
