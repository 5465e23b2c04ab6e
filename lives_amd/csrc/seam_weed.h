// seam_weed.h -- the host's plants as the layer seam sees them (definitions: seam_weed.cpp): the bound leaf accessors and the host's allocator, the palette
// predicates, the Layer snapshot of a weed_layer_t's leaves, and the new host planes a seam call allocates, commits or drops.  Nothing here knows about the
// device: the one lgpu_* call of this unit is lgpu_calc_rowstrides (host arithmetic).
// The seam's units (seam_weed, seam_resident, seam_lazy, layer_seam.cpp) share their internals through namespace seam, declared with hidden visibility: calls
// between the units bind directly (no PLT) and none of these names reaches the library's dynamic symbol table.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/lives_gpu.h"
#include "../../include/lives_gpu_layer.h"

#pragma GCC visibility push(hidden)
namespace seam {

extern lives_gpu_weed_api g_api;
extern weed_leaf_get_flags_f g_leaf_get_flags;      // optional, lives_gpu_bind_leaf_get_flags
extern lives_gpu_prefs g_prefs;

constexpr const char *kLeafHostFlags = "host_flags";          // LIVES_LEAF_HOST_FLAGS (src/colourspace.h:37)
constexpr const char *kLeafContiguous = "host_contiguous";    // LIVES_LEAF_PIXEL_DATA_CONTIGUOUS (:33)
constexpr const char *kLeafOpaque = "host_gpu_opaque";        // the host's word that every pixel of the layer's frame has alpha 255 (lives_gpu_layer_set_opaque)
constexpr const char *kLeafResident = "host_gpu_resident";    // this library's private leaf (host_* convention, src/effects-weed.h:80-119)

inline bool bound() { return g_api.leaf_get && g_api.leaf_set && g_api.leaf_num_elements && g_api.leaf_delete; }
void *palloc(size_t n, bool zeroed = true);
void pfree(void *p);

inline bool has_leaf(weed_plant_t *p, const char *k) { return g_api.leaf_num_elements(p, k) > 0; }
inline int get_int(weed_plant_t *p, const char *k, int dflt, int idx = 0) {
  int32_t v = dflt;
  if (g_api.leaf_get(p, k, (weed_size_t)idx, &v) != WEED_SUCCESS) return dflt;
  return v;
}
inline void set_int(weed_plant_t *p, const char *k, int v) { int32_t x = v; g_api.leaf_set(p, k, WEED_SEED_INT, 1, &x); }
inline void set_bool(weed_plant_t *p, const char *k, int v) { int32_t x = v; g_api.leaf_set(p, k, WEED_SEED_BOOLEAN, 1, &x); }

inline bool pal_is_rgb(int p) { return p >= WEED_PALETTE_RGB24 && p <= WEED_PALETTE_ARGB32; }
inline bool pal_is_planar_yuv(int p) { return p == WEED_PALETTE_YUV420P || p == WEED_PALETTE_YVU420P || p == WEED_PALETTE_YUV422P || p == WEED_PALETTE_YUV444P || p == WEED_PALETTE_YUVA4444P; }
inline bool pal_is_yuv(int p) {
  return pal_is_planar_yuv(p) || p == WEED_PALETTE_UYVY || p == WEED_PALETTE_YUYV || p == WEED_PALETTE_YUV888 || p == WEED_PALETTE_YUVA8888 || p == WEED_PALETTE_YUV411;
}
inline bool pal_is_444(int p) { return p == WEED_PALETTE_YUV444P || p == WEED_PALETTE_YUVA4444P; }
inline bool pal_alpha_first(int p) { return p == WEED_PALETTE_ARGB32; }
inline bool pal_alpha_last(int p) { return p == WEED_PALETTE_RGBA32 || p == WEED_PALETTE_BGRA32; }
inline bool pal_has_alpha(int p) { return pal_alpha_first(p) || pal_alpha_last(p) || p == WEED_PALETTE_YUVA8888 || p == WEED_PALETTE_YUVA4444P; }
inline bool pal_red_first(int p) { return p == WEED_PALETTE_RGB24 || p == WEED_PALETTE_RGBA32 || p == WEED_PALETTE_ARGB32; }
inline int pal_psize(int p) { return (p == WEED_PALETTE_RGB24 || p == WEED_PALETTE_BGR24) ? 3 : pal_is_rgb(p) ? 4 : pal_is_planar_yuv(p) ? 1 : 0; }
inline int pal_order(int p) { return pal_alpha_first(p) ? 2 : pal_red_first(p) ? 0 : 1; }      // an RGB palette's channel order in the kernels' numbers: 0 RGB, 1 BGR, 2 ARGB

// ---- a layer as this file sees it ------------------------------------------------------------------------------
struct Layer {
  weed_plant_t *plant;
  int pal, width, height, nplanes;
  int rs[4];
  uint8_t *pd[4];
  int clamping, subspace, sampling, gamma, flags;
  bool contiguous;
};

inline int plane_w(const Layer &l, int p) { return (p == 0 || pal_is_444(l.pal)) ? l.width : l.width >> 1; }
inline int plane_h(const Layer &l, int p) { return (p == 0 || pal_is_444(l.pal) || l.pal == WEED_PALETTE_YUV422P) ? l.height : l.height >> 1; }      // (not plane_rows: a layer with more planes than its palette has is walked by the leaf's count, and there the two differ)
// rows of plane p of a (pal, height) frame, for every p below the palette's plane count
inline int plane_rows(int pal, int height, int p) {
  return (!pal_is_planar_yuv(pal) || p == 0 || p == 3 || pal_is_444(pal) || pal == WEED_PALETTE_YUV422P) ? height : height >> 1;
}

bool read_layer(weed_plant_t *plant, Layer *l);
void free_host_planes(const Layer &l);              // the layer's host planes go back through the host's allocator (free_planes without the table)
void delete_yuv_leaves(weed_plant_t *layer);        // conv_done of a conversion that ends at an RGB palette

void apply_const_rowstrides(weed_plant_t *layer, int n, int *rs);
// new host planes for (pal, width, height) with the reference's rowstride rule; one block for planar ("contiguous")
struct NewPlanes { int n; int rs[4]; uint8_t *pd[4]; size_t sz[4]; };
void swap_chroma_planes(int pal, NewPlanes *np);
int take_alignment(int forced);
bool alloc_planes(int pal, int width, int height, int alignment, NewPlanes *np, weed_plant_t *fixed_from = nullptr, bool zeroed = false);
void commit_planes(weed_plant_t *plant, int pal, int width, int height, const NewPlanes &np);
void drop_new_planes(const NewPlanes &np);

int k3_fmt(int pal);
int k4_fmt(int pal);

}  // namespace seam
#pragma GCC visibility pop
