// seam_weed.cpp -- the host's plants (seam_weed.h): what the host bound, a layer's leaves read into a Layer, and the host planes of a new frame
// (rowstrides by the reference's rule, calc_rowstrides src/colourspace.c:11252-11366; one block for planar palettes) allocated, committed to the leaves or dropped.
#include <stdlib.h>
#include <string.h>
#include "seam_weed.h"

#pragma GCC visibility push(hidden)
namespace seam {

lives_gpu_weed_api g_api = {};
weed_leaf_get_flags_f g_leaf_get_flags = nullptr;      // optional, lives_gpu_bind_leaf_get_flags
lives_gpu_prefs g_prefs = {1, 0, 2, 1.4, 0};

// zeroed = false: every byte of the block is about to be overwritten (a download of whole planes, or -- pinned layer -- the bytes are stale by contract
// until lives_gpu_layer_sync() writes whole planes): glibc's calloc memsets recycled heap memory, ~60 us for a 1080p RGBA plane, which was the largest
// single item of a seam call's host time (tools/bench_seam.py; profiles/r02/seam_bench.txt)
void *palloc(size_t n, bool zeroed) {
  if (g_api.pixel_alloc) return g_api.pixel_alloc(n);
  return zeroed ? calloc(1, n ? n : 1) : malloc(n ? n : 1);
}
void pfree(void *p) { if (!p) return; if (g_api.pixel_free) g_api.pixel_free(p); else free(p); }

bool read_layer(weed_plant_t *plant, Layer *l) {
  if (!plant || !bound()) return false;
  l->plant = plant;
  l->pal = get_int(plant, WEED_LEAF_CURRENT_PALETTE, 0);
  l->width = get_int(plant, WEED_LEAF_WIDTH, 0);
  l->height = get_int(plant, WEED_LEAF_HEIGHT, 0);
  l->nplanes = (int)g_api.leaf_num_elements(plant, WEED_LEAF_PIXEL_DATA);
  if (l->nplanes < 1 || l->nplanes > 4 || (int)g_api.leaf_num_elements(plant, WEED_LEAF_ROWSTRIDES) < l->nplanes) return false;
  for (int i = 0; i < 4; i++) { l->rs[i] = 0; l->pd[i] = nullptr; }
  for (int i = 0; i < l->nplanes; i++) {
    l->rs[i] = get_int(plant, WEED_LEAF_ROWSTRIDES, 0, i);
    void *v = nullptr;
    g_api.leaf_get(plant, WEED_LEAF_PIXEL_DATA, (weed_size_t)i, &v);
    l->pd[i] = (uint8_t *)v;
  }
  if (!l->pd[0] || l->width <= 0 || l->height <= 0) return false;
  l->clamping = get_int(plant, WEED_LEAF_YUV_CLAMPING, -1);
  l->subspace = get_int(plant, WEED_LEAF_YUV_SUBSPACE, WEED_YUV_SUBSPACE_YUV);
  l->sampling = get_int(plant, WEED_LEAF_YUV_SAMPLING, WEED_YUV_SAMPLING_DEFAULT);
  l->gamma = get_int(plant, WEED_LEAF_GAMMA_TYPE, WEED_GAMMA_UNKNOWN);
  l->flags = get_int(plant, kLeafHostFlags, 0);
  l->contiguous = get_int(plant, kLeafContiguous, 0) != 0;
  return true;
}

void free_host_planes(const Layer &l) {
  if (l.contiguous) pfree(l.pd[0]);
  else for (int i = 0; i < l.nplanes; i++) pfree(l.pd[i]);
}
void delete_yuv_leaves(weed_plant_t *layer) {
  g_api.leaf_delete(layer, WEED_LEAF_YUV_CLAMPING);                          // conv_done (:13881-13884)
  g_api.leaf_delete(layer, WEED_LEAF_YUV_SUBSPACE);
  g_api.leaf_delete(layer, WEED_LEAF_YUV_SAMPLING);
}

// fixed rowstrides (:11268-11275): a "new_rowstrides" leaf, or rowstrides flagged LIVES_FLAG_CONST_VALUE (1 << 16, src/main.h:127); taken per
// plane when computed <= fixed < 2 * computed (the reference's integer `constrs[i] / rs[i]` between .75 and 1.25, :11358-11363)
void apply_const_rowstrides(weed_plant_t *layer, int n, int *rs) {
  if (!layer || !bound()) return;
  const char *key = nullptr;
  if (has_leaf(layer, "new_rowstrides")) key = WEED_LEAF_ROWSTRIDES;        // the reference reads the rowstrides leaf in both cases (:11269, :11273)
  else if (g_leaf_get_flags && has_leaf(layer, WEED_LEAF_ROWSTRIDES) && (g_leaf_get_flags(layer, WEED_LEAF_ROWSTRIDES) & (1 << 16))) key = WEED_LEAF_ROWSTRIDES;
  if (!key) return;
  const int have = (int)g_api.leaf_num_elements(layer, key);
  for (int i = 0; i < n && i < have; i++) {
    int32_t c = 0;
    if (g_api.leaf_get(layer, key, (weed_size_t)i, &c) != WEED_SUCCESS || rs[i] <= 0) continue;
    const int q = c / rs[i];
    if (q >= .75 && q <= 1.25) rs[i] = c;
  }
}

// THREADVAR(rowstride_alignment_hint) of the calling thread as calc_rowstrides consumes it (:11285-11297): a value >= 4 applies to the next
// allocation only, -1 (compact rows: what v1 playback plugins and the transcoder ask for, src/player.c:1355-1356, src/transcode.c:42) stays until
// the caller resets it.  The host forwards its own thread variable with lives_gpu_set_rowstride_alignment_hint(); the reference also remembers
// the last alignment used as the thread's new default (:11295) -- not mirrored: that default belongs to LiVES' own allocations.
static thread_local int t_rs_hint = 0;
int take_alignment(int forced) {
  if (forced) { t_rs_hint = 0; return forced; }      // resize_layer overwrites the hint with 16 and the allocation consumes it (:14989)
  const int h = t_rs_hint;
  if (h != -1) t_rs_hint = 0;
  return h;
}
bool alloc_planes(int pal, int width, int height, int alignment, NewPlanes *np, weed_plant_t *fixed_from, bool zeroed) {
  np->n = lgpu_calc_rowstrides(width, pal, take_alignment(alignment), np->rs);
  if (np->n < 1) return false;
  apply_const_rowstrides(fixed_from, np->n, np->rs);
  size_t tot = 0;
  for (int i = 0; i < np->n; i++) {
    np->sz[i] = (size_t)np->rs[i] * plane_rows(pal, height, i);
    tot += np->sz[i];
  }
  uint8_t *blk = (uint8_t *)palloc(tot + 64, zeroed);     // + EXTRA_BYTES-style slack (reference loops read a few bytes past the end)
  if (!blk) return false;
  if (!zeroed) memset(blk + tot, 0, 64);
  size_t off = 0;
  for (int i = 0; i < np->n; i++) { np->pd[i] = blk + off; off += np->sz[i]; }
  return true;
}
void swap_chroma_planes(int pal, NewPlanes *np) {
  if (pal == WEED_PALETTE_YVU420P) { uint8_t *t = np->pd[1]; np->pd[1] = np->pd[2]; np->pd[2] = t; }   // swap_chroma_planes (:13890)
}
void commit_planes(weed_plant_t *plant, int pal, int width, int height, const NewPlanes &np) {
  set_int(plant, WEED_LEAF_CURRENT_PALETTE, pal);
  set_int(plant, WEED_LEAF_WIDTH, width);
  set_int(plant, WEED_LEAF_HEIGHT, height);
  int32_t rs[4];
  void *pd[4];
  for (int i = 0; i < np.n; i++) { rs[i] = np.rs[i]; pd[i] = np.pd[i]; }
  g_api.leaf_set(plant, WEED_LEAF_ROWSTRIDES, WEED_SEED_INT, (weed_size_t)np.n, rs);
  g_api.leaf_set(plant, WEED_LEAF_PIXEL_DATA, WEED_SEED_VOIDPTR, (weed_size_t)np.n, pd);
  if (np.n > 1) set_bool(plant, kLeafContiguous, WEED_TRUE); else g_api.leaf_delete(plant, kLeafContiguous);
}
void drop_new_planes(const NewPlanes &np) { pfree(np.pd[0]); }       // one block (alloc_planes)

int k3_fmt(int pal) {
  switch (pal) {
  case WEED_PALETTE_YUV888: case WEED_PALETTE_YUVA8888: return 0;
  case WEED_PALETTE_YUV444P: case WEED_PALETTE_YUVA4444P: return 1;
  case WEED_PALETTE_UYVY: return 2;
  case WEED_PALETTE_YUYV: return 3;
  default: return -1;
  }
}
int k4_fmt(int pal) {
  switch (pal) {
  case WEED_PALETTE_YUV420P: case WEED_PALETTE_YVU420P: return 4;
  case WEED_PALETTE_YUV422P: return 5;
  default: return k3_fmt(pal);
  }
}

}  // namespace seam
#pragma GCC visibility pop
using namespace seam;

extern "C" {
void lives_gpu_set_rowstride_alignment_hint(int hint) { t_rs_hint = hint; }
int lives_gpu_get_rowstride_alignment_hint(void) { return t_rs_hint; }
}  // extern "C"
