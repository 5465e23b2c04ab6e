// seam_lazy.cpp -- deferred programs (seam_lazy.h; the rationale stands there, "deferred execution on pinned layers"): recording a stage on a plane's pending
// program, routing a group of programs of one shape to the one-launch forms of the frame-level API (lives_gpu.h) and running what those refuse stage by stage;
// and the public entry points about programs: lives_gpu_set_deferred, lives_gpu_set_flat_yuv, lives_gpu_set_pending_layer2, lives_gpu_deferred_stats[_n],
// lives_gpu_layers_flush, lives_gpu_deferred_blend_chroma.
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <unordered_set>
#include <vector>
#include "seam_lazy.h"

#pragma GCC visibility push(hidden)
namespace seam {

std::atomic<int> g_deferred{1};
std::atomic<unsigned long long> g_lz_recorded{0}, g_lz_chain_launches{0}, g_lz_chain_tracks{0}, g_lz_staged{0};      // lives_gpu_deferred_stats
std::atomic<unsigned long long> g_lz_yuv_recorded{0}, g_lz_yuv_launches{0}, g_lz_yuv_tracks{0}, g_lz_yuv_pre{0};        // lives_gpu_deferred_stats_n [4..7]
std::atomic<unsigned long long> g_lz_sink_recorded{0}, g_lz_sink_launches{0}, g_lz_sink_tracks{0}, g_lz_sink_fused{0};    // lives_gpu_deferred_stats_n [8..11]
std::atomic<unsigned long long> g_lz_transcode{0};                                                                          // lives_gpu_deferred_stats_n [12]
std::atomic<unsigned long long> g_lz_flat_launches{0}, g_lz_flat_tracks{0};                                                     // lives_gpu_deferred_stats_n [13..14]
std::atomic<unsigned long long> g_lz_l2_recorded{0}, g_lz_mix_launches{0}, g_lz_mix_tracks{0}, g_lz_l2_first{0};               // lives_gpu_deferred_stats_n [15..18]
std::atomic<int> g_pending_l2{0};   // lives_gpu_set_pending_layer2: 0 a blend runs a pending layer 2 when it is recorded (today), 1 / 2 / 3 it stays pending (the flush folds by MIX_FOLD_PAIRS / always / never)
std::atomic<int> g_flat_yuv{0};     // lives_gpu_set_flat_yuv: unscaled YUV groups take the one-launch forms of flat.hip (off until the default is flipped with the tests' expectations)
std::mutex g_lazy_mu;               // one program (group) runs at a time; never taken with a table lock held

static void lazy_unread(Lazy *z) {          // (no lock held) the program no longer reads its layer 2
  if (!z->blend || !z->l2h) return;
  res_update(z->l2h, [z](Dev *e) {
    if (e && e->lazy_readers > 0) e->lazy_readers--;
    z->l2h = nullptr;
  });
}
// the program is over: its source planes go back to the pool.  ran (lazy_run_group): launches on the calling thread's stream have just read them -- the three planes
// of a YUV program go back with the streams that read them kept (a later taker waits for the writer AND these readers), an RGBA frame with that stream as its last use
static void lazy_free(Lazy *z, bool ran) {
  Dev src = z->src, yu = z->yu, yv = z->yv;
  const bool yuv = z->yuv;
  delete z;
  if (ran && yuv) { note_use(src, false); note_use(yu, false); note_use(yv, false); }
  else if (ran) { src.stream = S(); src.nr = 0; }
  pool_give(src);
  if (yuv) { pool_give(yu); pool_give(yv); }
}
void lazy_discard(Lazy *z) {
  if (!z) return;
  if (z->sink)                          // the entries of the program's other planes point at it too: they go with it (the caller has taken its own out already)
    for (int p = 0; p < z->snp; p++) res_take_if(z->sph[p], [z](const Dev &e) { return e.lazy == z; });
  lazy_unread(z);
  lazy_free(z, false);
}
// (g_lazy_mu held) the program that the pending layer 2 of z still is; nullptr: z's layer 2 is not pending -- or no longer: it has run meanwhile (somebody needed
// its pixels), so they are taken as a blend recorded against a resident plane has them
static Lazy *lazy_l2_program(Lazy *z) {
  if (!z->l2pend) return nullptr;
  Dev e;
  const bool there = res_peek(z->l2h, &e);
  if (there && e.lazy) return e.lazy;
  z->l2 = there ? e : Dev();          // (no entry at all: cannot happen, a plane with readers is not dropped before they have run)
  z->l2pend = false;
  return nullptr;
}
// (g_lazy_mu held where a layer 2 is pending) one launch can carry both: the same stages on frames of the same geometry and, behind a pending layer 2, layer-2
// programs of one shape as well
static bool lazy_same_shape(Lazy *a, Lazy *b) {
  Lazy *const a2 = lazy_l2_program(a), *const b2 = lazy_l2_program(b);
  if ((a2 != nullptr) != (b2 != nullptr) || (a2 && a2 != b2 && !lazy_same_shape(a2, b2))) return false;
  return a->sw == b->sw && a->sh == b->sh && a->srs == b->srs && a->swap == b->swap && a->scale == b->scale && a->dw == b->dw && a->dh == b->dh &&
         a->interp == b->interp && a->opaque == b->opaque && a->canvas == b->canvas && a->nw == b->nw && a->nh == b->nh && a->ox == b->ox && a->oy == b->oy && a->blend == b->blend &&
         a->l2rs == b->l2rs &&          /* (not the blend amount: every track of a launch has its own, lgpu_chain_amounts) */ a->lut == b->lut && (!a->lut || !memcmp(a->lut8, b->lut8, 256)) && a->w == b->w && a->h == b->h && a->rs == b->rs &&
         a->yuv == b->yuv && (!a->yuv || (a->yfmt == b->yfmt && !memcmp(a->ystr, b->ystr, sizeof a->ystr) && a->usz == b->usz && a->vsz == b->vsz && a->order == b->order && a->which == b->which && a->quality == b->quality)) &&
         a->sink == b->sink && (!a->sink || (a->sfmt == b->sfmt && a->swhich == b->swhich && a->sorder == b->sorder && a->snp == b->snp && a->sww == b->sww && a->shh == b->shh &&
                                             !memcmp(a->sors, b->sors, sizeof a->sors)));
}
// one program, stage by stage through stream-ordered scratch frames, into out (the plane's rowstride)
static int lazy_run_staged(const Lazy *z, uint8_t *out, const uint8_t *src, int srs) {
  const uint8_t *cur = src;
  int cw = z->sw, ch = z->sh, crs = srs, rc = LGPU_OK;
  void *tmp[3] = {nullptr, nullptr, nullptr};
  int nt = 0;
  const int last_geo = z->canvas ? LZ_CANVAS : z->scale ? LZ_SCALE : LZ_SWAP;
  auto target = [&](int stage, int w, int h, uint8_t **dst, int *drs) -> int {       // where a geometric stage writes: the plane itself for the last one
    if (stage == last_geo) { *dst = out; *drs = z->rs; return LGPU_OK; }
    const int r = lgpu_malloc_ordered(&tmp[nt], (size_t)w * 4 * h + 64, S());
    if (r) return r;
    *dst = (uint8_t *)tmp[nt++]; *drs = w * 4;
    return LGPU_OK;
  };
  uint8_t *dst = nullptr;
  int drs = 0;
  if (!z->swap && !z->scale && !z->canvas) rc = lgpu_copy_rows(out, z->rs, cur, crs, cw * 4, ch, S());      // no geometric stage: the in-place stages work on a copy
  if (!rc && z->swap) {
    if (!(rc = target(LZ_SWAP, cw, ch, &dst, &drs))) rc = lgpu_swizzle(LGPU_SWAP3POSTALPHA, 0, cur, crs, dst, drs, cw, ch, nullptr, S());
    cur = dst; crs = drs;
  }
  if (!rc && z->scale) {
    if (!(rc = target(LZ_SCALE, z->dw, z->dh, &dst, &drs))) rc = lgpu_pixbuf_scale(cur, crs, cw, ch, dst, drs, z->dw, z->dh, 4, z->interp | (z->opaque ? LGPU_INTERP_OPAQUE : 0), S());
    cur = dst; crs = drs; cw = z->dw; ch = z->dh;
  }
  if (!rc && z->canvas) {
    const uint8_t black[4] = {0, 0, 0, 255};
    if (!(rc = target(LZ_CANVAS, z->nw, z->nh, &dst, &drs))) rc = lgpu_letterbox_at(cur, crs, cw, ch, dst, drs, z->nw, z->nh, 4, black, z->ox, z->oy, S());
    cur = dst; crs = drs; cw = z->nw; ch = z->nh;
  }
  if (!rc && z->blend) rc = lgpu_blend_chroma(out, z->rs, (const uint8_t *)z->l2.d, z->l2rs, out, z->rs, z->w, z->h, 4, 0, z->bf, S());
  if (!rc && z->lut) rc = lgpu_gamma_apply(out, z->rs, 0, 0, z->w, z->h, 4, 0, z->lut8, S());
  for (int i = 0; i < nt; i++) lgpu_free_ordered(tmp[i], S());
  return rc;
}
// ---- a group of programs of one shape as the arguments of the one-launch forms.  Every public struct is filled from a Lazy HERE and nowhere else. ----
// to_sink: the group ends at a YUV sink -- no destination rowstride, no layer-2 rowstride without a blend, no OPAQUE word, and the source rowstride is the luma
// plane's behind YUV planes.  An RGBA destination keeps the recorded frame's rowstride as irow whatever the source (the YUV forms do not read it)
static lgpu_chain_params lazy_params(const Lazy *z, bool to_sink) {
  lgpu_chain_params pr;
  memset(&pr, 0, sizeof pr);
  pr.sw = z->sw; pr.sh = z->sh; pr.dw = z->scale ? z->dw : z->sw; pr.dh = z->scale ? z->dh : z->sh;
  pr.swap_rb = z->swap ? 1 : 0; pr.interp = (z->scale ? z->interp : 0) | LGPU_INTERP_PIXBUF | (z->blend ? 0 : LGPU_INTERP_NOBLEND); pr.do_blur = 0; pr.use_lut = z->lut ? 1 : 0;
  if (z->lut) memcpy(pr.lut8, z->lut8, 256);
  if (to_sink) { pr.irow = z->yuv ? z->ystr[0] : z->srs; pr.irow2 = z->blend ? z->l2rs : 0; pr.orow = 0; }
  else {
    pr.irow = z->srs; pr.irow2 = z->blend ? z->l2rs : z->rs; pr.orow = z->rs; pr.bf = z->bf;
    if (z->scale && z->opaque) pr.interp |= LGPU_INTERP_OPAQUE;
  }
  return pr;
}
// the decoded frames a YUV program starts from: lgpu_yuv_source (4:2:0 planes; flags stay 0), or lgpu_yuv422_source -- the same description with the format beside
// it -- for a YUV422P / UYVY / YUYV group (lgpu_chain_flat_yuv422)
template <class Source> Source lazy_source(const Lazy *z) {
  Source s;
  memset(&s, 0, sizeof s);
  s.istrides[0] = z->ystr[0]; s.istrides[1] = z->ystr[1]; s.istrides[2] = z->ystr[2]; s.u_size = z->usz; s.v_size = z->vsz;
  s.out_order = z->order; s.which_tables = z->which; s.pb_quality = z->quality;
  if constexpr (std::is_same<Source, lgpu_yuv422_source>::value) s.in_fmt = z->yfmt;
  return s;
}
static lgpu_chain_sink lazy_sink(const Lazy *z) {
  lgpu_chain_sink sk;
  memset(&sk, 0, sizeof sk);
  sk.out_fmt = z->sfmt; sk.which_tables = z->swhich; sk.in_order = z->sorder;
  for (int p = 0; p < z->snp; p++) sk.orow[p] = z->sors[p];
  return sk;
}
static std::vector<uint8_t> lazy_amounts(Lazy *const *zs, int n) {
  std::vector<uint8_t> am((size_t)n);
  for (int i = 0; i < n; i++) am[(size_t)i] = (uint8_t)zs[i]->bf;
  return am;
}
// the per-track arrays.  Destinations: outp[i] (one RGBA plane per track) or, for a sink, souts[i][0 .. snp)
static std::vector<lgpu_chain_track> lazy_tracks(Lazy *const *zs, int n, const uint8_t *const *srcp, uint8_t *const *outp) {
  std::vector<lgpu_chain_track> tr((size_t)n);
  for (int i = 0; i < n; i++) { tr[(size_t)i].src_d = srcp[i]; tr[(size_t)i].layer2_d = (const uint8_t *)zs[i]->l2.d; tr[(size_t)i].dst_d = outp[i]; }
  return tr;
}
static std::vector<lgpu_chain_yuv_track> lazy_yuv_tracks(Lazy *const *zs, int n, uint8_t *const *outp) {
  std::vector<lgpu_chain_yuv_track> yt((size_t)n);
  for (int i = 0; i < n; i++) {
    lgpu_chain_yuv_track &t = yt[(size_t)i];
    t.y_d = (const uint8_t *)zs[i]->src.d; t.u_d = (const uint8_t *)zs[i]->yu.d; t.v_d = (const uint8_t *)zs[i]->yv.d;
    t.layer2_d = (const uint8_t *)zs[i]->l2.d; t.dst_d = outp[i];
  }
  return yt;
}
static std::vector<lgpu_chain_yuv_sink_track> lazy_yuv_sink_tracks(Lazy *const *zs, int n, uint8_t *const *outp, Dev (*souts)[3]) {
  std::vector<lgpu_chain_yuv_sink_track> tr((size_t)n);
  for (int i = 0; i < n; i++) {
    lgpu_chain_yuv_sink_track &t = tr[(size_t)i];
    memset(&t, 0, sizeof t);
    t.y_d = (const uint8_t *)zs[i]->src.d; t.u_d = (const uint8_t *)zs[i]->yu.d; t.v_d = (const uint8_t *)zs[i]->yv.d;
    t.layer2_d = (const uint8_t *)zs[i]->l2.d;
    if (souts) for (int p = 0; p < zs[0]->snp; p++) t.dst_d[p] = (uint8_t *)souts[i][p].d;
    else t.dst_d[0] = outp[i];
  }
  return tr;
}
static std::vector<lgpu_chain_sink_track> lazy_sink_tracks(Lazy *const *zs, int n, Dev (*souts)[3]) {
  std::vector<lgpu_chain_sink_track> tr((size_t)n);
  for (int i = 0; i < n; i++) {
    lgpu_chain_sink_track &t = tr[(size_t)i];
    memset(&t, 0, sizeof t);
    t.src_d = (const uint8_t *)zs[i]->src.d; t.layer2_d = (const uint8_t *)zs[i]->l2.d;
    for (int p = 0; p < zs[0]->snp; p++) t.dst_d[p] = (uint8_t *)souts[i][p].d;
  }
  return tr;
}
// the launches of this thread's stream wait for whoever wrote the planes a program reads
static void lazy_await(const Lazy *z) {
  await(z->src, false);
  if (z->yuv) { await(z->yu, false); await(z->yv, false); }
  if (z->blend) await(z->l2, false);
}
// What a one-launch route answered: LGPU_OK -- the group is done (true) and the route's counters move: the chain's always, those of the kinds it names beside them,
// by the call's `launches` and n tracks; LGPU_E_BADARG / LGPU_E_UNSUPPORTED -- the shape is not the form's, the next route takes the group; anything else is the
// group's error (*rc)
enum { RT_YUV = 1, RT_SINK = 2, RT_FLAT = 4, RT_TRANSCODE = 8, RT_MIX = 16 };
static bool lazy_route(int crc, unsigned kinds, int launches, int n, int *rc) {
  if (crc != LGPU_OK) {
    if (crc != LGPU_E_BADARG && crc != LGPU_E_UNSUPPORTED) *rc = crc;
    return false;
  }
  const unsigned long long nl = (unsigned long long)launches, nt = (unsigned long long)n;
  g_lz_chain_launches += nl; g_lz_chain_tracks += nt;
  if (kinds & RT_YUV) { g_lz_yuv_launches += nl; g_lz_yuv_tracks += nt; }
  if (kinds & RT_SINK) { g_lz_sink_launches += nl; g_lz_sink_tracks += nt; g_lz_sink_fused += nl; }
  if (kinds & RT_FLAT) { g_lz_flat_launches += nl; g_lz_flat_tracks += nt; }
  if (kinds & RT_TRANSCODE) g_lz_transcode += nl;
  if (kinds & RT_MIX) { g_lz_mix_launches += nl; g_lz_mix_tracks += nt; }
  return true;
}
// the RGBA stages of n programs of one shape into outp[i] (rowstride z0->rs): one fused launch where the shape allows, else stage by stage.  The routes, in order:
//   1. lgpu_chain_yuv420p           YUV 4:2:0 planes, scaled
//   2. lgpu_chain_flat_yuv422 / lgpu_chain_flat_yuv420p   YUV planes that keep their size, something behind the conversion, lives_gpu_set_flat_yuv(1)
//   3. the conversion as a launch of its own (a YUV group that took neither), then
//   4. lgpu_chain_amounts           every RGBA shape
//   5. lazy_run_staged              track by track (more than 64 tracks, SEAM_STAGED, a shape lgpu_chain_amounts refuses)
static int lazy_run_rgba(Lazy *const *zs, int n, uint8_t *const *outp) {
  const Lazy *z0 = zs[0];
  const size_t bytes = (size_t)z0->rs * z0->h;
  int rc = LGPU_OK;
  for (int i = 0; i < n; i++) {
    lazy_await(zs[i]);
    if (z0->rs != z0->w * 4) rc = rc ? rc : lgpu_fill(outp[i], 0, bytes, S());      // the row padding of a fresh plane is zero (calloc in the eager path)
  }
  bool done = false;
  const bool staged = lgpu_tuning_get("SEAM_STAGED") > 0;
  const bool one_launch = !staged && n <= LGPU_CHAIN_MAX_TRACKS;
  // the RGBA frames the later stages start from: the recorded source planes, or -- behind a YUV stage that is not fused -- converted scratch frames
  std::vector<const uint8_t *> srcp((size_t)n);
  for (int i = 0; i < n; i++) srcp[(size_t)i] = (const uint8_t *)zs[i]->src.d;
  int srow = z0->srs;
  void *scr = nullptr;
  lgpu_chain_params pr = lazy_params(z0, false);
  const std::vector<uint8_t> amounts = lazy_amounts(zs, n);
  const uint8_t *const blend_amounts = z0->blend ? amounts.data() : nullptr;
  const lgpu_canvas cv = {z0->nw, z0->nh, z0->ox, z0->oy};
  const lgpu_canvas *const cvp = z0->canvas ? &cv : nullptr;
  if (!rc && z0->yuv) {
    const int strides[3] = {z0->ystr[0], z0->ystr[1], z0->ystr[2]};
    if (one_launch && z0->scale && z0->yfmt == 4) {
      // the one-launch form: the conversion rides in the chain's loads (lgpu_chain_yuv420p, 4:2:0 planes only); every other shape is refused there and takes the two launches below
      const lgpu_yuv_source ys = lazy_source<lgpu_yuv_source>(z0);
      const std::vector<lgpu_chain_yuv_track> yt = lazy_yuv_tracks(zs, n, outp);
      done = lazy_route(lgpu_chain_yuv420p(&pr, &ys, cvp, yt.data(), n, blend_amounts, S()), RT_YUV, 1, n, &rc);
    }
    // lives_gpu_set_flat_yuv(1): a group that keeps its size (letterboxed or not) with anything behind the conversion takes lgpu_chain_flat_yuv420p, ONE launch and no
    // converted frame; a conversion that is all there is stays with K2's own kernel below (the same bytes either way, and that kernel is the faster converter).
    // The same from YUV422P / UYVY / YUYV frames: lgpu_chain_flat_yuv422.  A refused shape takes the two launches below
    if (!rc && !done && one_launch && !z0->scale && g_flat_yuv.load() && (z0->swap || z0->canvas || z0->blend || z0->lut)) {
      if (z0->yfmt != 4) {
        const lgpu_yuv422_source y4 = lazy_source<lgpu_yuv422_source>(z0);
        const std::vector<lgpu_chain_yuv_sink_track> yt = lazy_yuv_sink_tracks(zs, n, outp, nullptr);
        done = lazy_route(lgpu_chain_flat_yuv422(&pr, &y4, cvp, nullptr, yt.data(), n, blend_amounts, S()), RT_FLAT, 1, n, &rc);
      } else {
        const lgpu_yuv_source ys = lazy_source<lgpu_yuv_source>(z0);
        const std::vector<lgpu_chain_yuv_track> yt = lazy_yuv_tracks(zs, n, outp);
        done = lazy_route(lgpu_chain_flat_yuv420p(&pr, &ys, cvp, yt.data(), n, blend_amounts, S()), RT_FLAT, 1, n, &rc);
      }
    }
    if (!rc && !done) {
      // two launches: the group's conversions in one batch (SEAM_STAGED: one call per track), then the RGBA program -- or straight into the planes when the
      // conversion is all there is
      const bool only = !z0->swap && !z0->scale && !z0->canvas && !z0->blend && !z0->lut;
      const size_t per = (size_t)z0->sw * 4 * z0->sh;
      if (!only && (rc = lgpu_malloc_ordered(&scr, per * (size_t)n + 64, S()))) scr = nullptr;
      std::vector<lgpu_yuv_frame> fr((size_t)n);
      for (int i = 0; i < n; i++) {
        fr[(size_t)i].y_d = (const uint8_t *)zs[i]->src.d; fr[(size_t)i].u_d = (const uint8_t *)zs[i]->yu.d; fr[(size_t)i].v_d = (const uint8_t *)zs[i]->yv.d;
        fr[(size_t)i].dst_d = only ? outp[i] : (uint8_t *)scr + (size_t)i * per;
      }
      const int orow = only ? z0->rs : z0->sw * 4;
      const int is_422 = z0->yfmt == 5 ? 1 : 0;
      if (z0->yfmt == 2 || z0->yfmt == 3) {
        // a packed frame: K3 (lgpu_yuv_to_rgb), LGPU_FX_MAX_FRAMES frames per batch
        const int irs[4] = {strides[0], 0, 0, 0};
        for (int i0 = 0; i0 < n && !rc; i0 += (staged ? 1 : LGPU_FX_MAX_FRAMES)) {
          const int m = staged ? 1 : std::min(n - i0, (int)LGPU_FX_MAX_FRAMES);
          const uint8_t *sp[LGPU_FX_MAX_FRAMES * 4];
          uint8_t *dp[LGPU_FX_MAX_FRAMES];
          memset(sp, 0, sizeof sp);
          for (int i = 0; i < m; i++) { sp[i * 4] = fr[(size_t)(i0 + i)].y_d; dp[i] = fr[(size_t)(i0 + i)].dst_d; }
          if (staged) rc = lgpu_yuv_to_rgb(sp, irs, z0->sw, z0->sh, z0->yfmt, 0, dp[0], orow, z0->order, 1, z0->which, S());
          else { rc = lgpu_yuv_to_rgb_batch(sp, irs, z0->sw, z0->sh, z0->yfmt, 0, dp, orow, z0->order, 1, z0->which, m, S()); if (!rc) g_lz_yuv_pre++; }
        }
      } else if (!rc && !staged && n <= LGPU_CHAIN_MAX_TRACKS) {
        rc = lgpu_yuv420p_to_rgb_batch(n, fr.data(), strides, z0->usz, z0->vsz, orow, z0->sw, z0->sh, 4, z0->order, is_422, z0->which, z0->quality, nullptr, 0, S());
        if (!rc) g_lz_yuv_pre++;
      } else
        for (int i = 0; i < n && !rc; i++)
          rc = lgpu_yuv420p_to_rgb(fr[(size_t)i].y_d, fr[(size_t)i].u_d, fr[(size_t)i].v_d, strides, z0->usz, z0->vsz, fr[(size_t)i].dst_d, orow, z0->sw, z0->sh, 4,
                                   z0->order, is_422, z0->which, z0->quality, nullptr, 0, S());
      if (only) done = true;
      for (int i = 0; i < n; i++) srcp[(size_t)i] = (const uint8_t *)fr[(size_t)i].dst_d;
      srow = z0->sw * 4;
      pr.irow = srow;
    }
  }
  // every shape: with or without a resize stage, with or without a blend (lgpu_chain_amounts); LGPU_SEAM_STAGED / lgpu_tuning_set("SEAM_STAGED", 1): the fallback walk, for tests
  if (!rc && !done && one_launch) {
    const std::vector<lgpu_chain_track> tr = lazy_tracks(zs, n, srcp.data(), outp);
    done = lazy_route(lgpu_chain_amounts(&pr, cvp, tr.data(), n, amounts.data(), S()), 0, 1, n, &rc);          // a shape the fused kernel does not take runs stage by stage below
  }
  if (!rc && !done)
    for (int i = 0; i < n && !rc; i++) { rc = lazy_run_staged(zs[i], outp[i], srcp[(size_t)i], srow); g_lz_staged++; }
  if (scr) lgpu_free_ordered(scr, S());
  return rc;
}
static int lazy_run_sink(Lazy *const *zs, int n, Dev (*souts)[3]);
static int lazy_run_group(Lazy *const *zs, const void *const *hs, int n);
#define FLAT_SINK_FORMATS(fmt) ((fmt) == 2 || (fmt) == 3 || (fmt) == 4)
// Which pairs (layer 1's format f1, layer 2's format f2: 4 YUV420P, 5 YUV422P, 2 UYVY, 3 YUYV; canvas: both layers letterboxed) mode 1 of
// lives_gpu_set_pending_layer2 folds into ONE lgpu_chain_flat_yuv_mix launch: those for which tools/bench_seam_transition.py shows the launch ahead of mode 3's two
// launches (the second layers' batched conversion, then the readers' flat launch) by more than the round-to-round spread of the latter.
// profiles/r17/seam_transition.md (16 x 1080p, convert -> chroma blend -> gamma, host clock around 8 ticks, five interleaved rounds; layer 2 over layer 1, one launch
// against two, the two launches' spread): YUV420P over YUV420P 548.1 us against 557.3 (spread 123.4), UYVY over YUV420P 524.4 against 542.0 (18.4), YUV420P over
// UYVY 530.9 against 530.2 (7.0), YUV422P over YUV422P 589.5 against 584.8 (20.1); to a UYVY sink 596.2 / 609.5 (17.3), 549.8 / 558.8 (30.7), 546.4 / 553.3 (14.8),
// 581.0 / 584.0 (118.6); 1440x1080 letterboxed into 1920x1080, YUV420P over YUV420P, 618.4 against 635.2 (28.8).  The tick is bound by the host's calls at this
// size, both forms are 34 to 58 us ahead of today's 17 launches and within each other's spread: NO pair is taken, mode 1 runs the second layers first for every
// pair until a measurement tells them apart.  The pairs not timed (YUYV, YVU420P, the other cross pairs) are not taken either.
#define MIX_FOLD_PAIRS(f1, f2, canvas) (false && (f1) && (f2) && (canvas))
// (g_lazy_mu held) may the group zs, whose layer 2 are the pending programs z2s, run as lgpu_chain_flat_yuv_mix[_canvas]?  The mode allows the pair, the flat route
// is on, SEAM_STAGED is off; layer 1 is a YUV program that keeps its size; layer 2 is a conversion alone, or a conversion letterboxed onto layer 1's canvas at layer
// 1's place; both frames have one size; layer 2 was converted into the byte order the blend works in; and no sink stands behind a canvas
static bool lazy_folds(Lazy *const *zs, Lazy *const *z2s, int n) {
  const Lazy *z1 = zs[0], *z2 = z2s[0];
  const int mode = g_pending_l2.load();
  if (mode == 0 || mode == 3 || !g_flat_yuv.load() || lgpu_tuning_get("SEAM_STAGED") > 0 || n > LGPU_CHAIN_MAX_TRACKS) return false;
  if (!z1->yuv || z1->scale || !z2->yuv || z2->scale || z2->swap || z2->lut || z2->blend || z2->sink) return false;
  if (z1->sw != z2->sw || z1->sh != z2->sh || z2->order != (z1->order ^ (z1->swap ? 1 : 0))) return false;
  if (z1->canvas != z2->canvas || (z1->canvas && (z1->nw != z2->nw || z1->nh != z2->nh || z1->ox != z2->ox || z1->oy != z2->oy))) return false;
  if (z1->sink && (z1->canvas || z1->sww != z1->w || z1->shh != z1->h || !FLAT_SINK_FORMATS(z1->sfmt))) return false;
  if (mode == 1 && !MIX_FOLD_PAIRS(z1->yfmt, z2->yfmt, z1->canvas)) return false;
  for (int i = 1; i < n; i++) if (z2s[i] != z2 && !lazy_same_shape(z2s[i], const_cast<Lazy *>(z2))) return false;
  return true;
}
static lgpu_yuv_layer_source lazy_layer_source(const Lazy *z) {
  lgpu_yuv_layer_source s;
  memset(&s, 0, sizeof s);
  s.in_fmt = z->yfmt; s.istrides[0] = z->ystr[0]; s.istrides[1] = z->ystr[1]; s.istrides[2] = z->ystr[2]; s.u_size = z->usz; s.v_size = z->vsz;
  s.out_order = z->order; s.which_tables = z->which; s.pb_quality = z->quality;
  return s;
}
// the fold: n programs of one shape and their pending layer-2 programs as ONE lgpu_chain_flat_yuv_mix (RGBA or a sink) or lgpu_chain_flat_yuv_mix_canvas per
// LGPU_CHAIN_MIX_TRACKS tracks, into outs[track][plane].  true: done.  false with *rc == LGPU_OK: the entry point refused the shape, nothing was enqueued and the
// layer-2 programs run first instead
static bool lazy_run_mix(Lazy *const *zs, Lazy *const *z2s, int n, Dev (*outs)[3], int *rc) {
  const Lazy *z0 = zs[0];
  const int np = z0->sink ? z0->snp : 1;
  const int row_bytes[3] = {z0->sink ? (z0->sfmt == 4 ? z0->sww : z0->sww * 2) : z0->w * 4, z0->sww >> 1, z0->sww >> 1};
  for (int i = 0; i < n; i++) {
    lazy_await(zs[i]);
    await(z2s[i]->src, false); await(z2s[i]->yu, false); await(z2s[i]->yv, false);          // the launch reads layer 2's source planes on this stream
    for (int p = 0; p < np && !*rc; p++)
      if ((z0->sink ? z0->sors[p] : z0->rs) != row_bytes[p]) *rc = lgpu_fill(outs[i][p].d, 0, z0->sink ? z0->sbytes[p] : (size_t)z0->rs * z0->h, S());      // the row padding of a fresh plane is zero
  }
  if (*rc) return false;
  const lgpu_chain_params pr = lazy_params(z0, z0->sink);
  const lgpu_yuv_layer_source s1 = lazy_layer_source(z0), s2 = lazy_layer_source(z2s[0]);
  const lgpu_chain_sink sk = lazy_sink(z0);
  const lgpu_canvas cv = {z0->nw, z0->nh, z0->ox, z0->oy};
  const std::vector<uint8_t> amounts = lazy_amounts(zs, n);
  std::vector<lgpu_chain_yuv_mix_track> tr((size_t)n);
  for (int i = 0; i < n; i++) {
    lgpu_chain_yuv_mix_track &t = tr[(size_t)i];
    memset(&t, 0, sizeof t);
    t.y_d = (const uint8_t *)zs[i]->src.d; t.u_d = (const uint8_t *)zs[i]->yu.d; t.v_d = (const uint8_t *)zs[i]->yv.d;
    t.y2_d = (const uint8_t *)z2s[i]->src.d; t.u2_d = (const uint8_t *)z2s[i]->yu.d; t.v2_d = (const uint8_t *)z2s[i]->yv.d;
    for (int p = 0; p < np; p++) t.dst_d[p] = (uint8_t *)outs[i][p].d;
  }
  const int crc = z0->canvas ? lgpu_chain_flat_yuv_mix_canvas(&pr, &s1, &s2, &cv, tr.data(), n, amounts.data(), S())
                             : lgpu_chain_flat_yuv_mix(&pr, &s1, &s2, z0->sink ? &sk : nullptr, tr.data(), n, amounts.data(), S());
  if (!lazy_route(crc, RT_FLAT | RT_MIX | (z0->sink ? RT_SINK : 0), (n + LGPU_CHAIN_MIX_TRACKS - 1) / LGPU_CHAIN_MIX_TRACKS, n, rc)) return false;
  for (int i = 0; i < n; i++) { note_use(z2s[i]->src, false); note_use(z2s[i]->yu, false); note_use(z2s[i]->yv, false); }      // (not table entries: the program owns them)
  return true;
}
// layer 2 first: the distinct pending layer-2 programs of a group run as groups of THEIR shape -- one batched conversion, one lgpu_chain_yuv420p launch without a
// blend, whatever lazy_run_group makes of them -- and become resident planes with their reader counts kept
static int lazy_run_l2_first(Lazy *const *z2s, const void *const *l2hs, int n) {
  std::vector<Lazy *> ps;
  std::vector<const void *> ph;
  for (int i = 0; i < n; i++)
    if (z2s[i] && std::find(ps.begin(), ps.end(), z2s[i]) == ps.end()) { ps.push_back(z2s[i]); ph.push_back(l2hs[i]); }
  std::vector<char> done(ps.size(), 0);
  for (size_t i = 0; i < ps.size(); i++) {
    if (done[i]) continue;
    std::vector<Lazy *> gz;
    std::vector<const void *> gh;
    for (size_t k = i; k < ps.size() && (int)gz.size() < LGPU_CHAIN_MAX_TRACKS; k++)
      if (!done[k] && (k == i || lazy_same_shape(ps[i], ps[k]))) { done[k] = 1; gz.push_back(ps[k]); gh.push_back(ph[k]); }
    const int rc = lazy_run_group(gz.data(), gh.data(), (int)gz.size());      // (ps[i] is gz[0]: it is not looked at again)
    if (rc) return rc;
    g_lz_l2_first += (unsigned long long)gz.size();
  }
  return LGPU_OK;
}
// run n pending programs of ONE shape (g_lazy_mu held by the caller; hs[i]: the host plane zs[i] is registered under; a program that ends in LZ_SINK names its planes itself, Lazy::sph).  Afterwards the planes are ordinary
// resident planes whose last writer is the calling thread's stream.  A group whose layer 2 is pending (Lazy::l2pend) is folded with it into one launch
// (lazy_folds, lazy_run_mix) -- the layer-2 programs then STAY pending, with one reader fewer -- or has its layer-2 programs run first (lazy_run_l2_first)
static int lazy_run_group(Lazy *const *zs, const void *const *hs, int n) {
  const Lazy *z0 = zs[0];
  const bool sink = z0->sink;
  const int np = sink ? z0->snp : 1;
  std::vector<Dev> outs((size_t)n * 3);                                               // [track][plane]
  int rc = LGPU_OK;
  std::vector<Lazy *> z2s((size_t)n);
  std::vector<const void *> l2hs((size_t)n);
  int npend = 0;
  for (int i = 0; i < n; i++) { z2s[(size_t)i] = lazy_l2_program(zs[i]); l2hs[(size_t)i] = zs[i]->l2h; npend += z2s[(size_t)i] ? 1 : 0; }
  const bool fold = npend == n && lazy_folds(zs, z2s.data(), n);
  auto l2_first = [&]() {
    const int r = lazy_run_l2_first(z2s.data(), l2hs.data(), n);
    if (r) return r;
    for (int i = 0; i < n; i++) if (lazy_l2_program(zs[i])) return (int)LGPU_E_BADARG;      // (cannot happen: each has just become a resident plane)
    npend = 0;
    return (int)LGPU_OK;
  };
  if (npend && !fold) rc = l2_first();
  if (rc) return rc;
  for (int i = 0; i < n && !rc; i++)
    for (int p = 0; p < np && !rc; p++)
      if (!pool_take(sink ? z0->sbytes[p] : (size_t)z0->rs * z0->h, &outs[(size_t)i * 3 + p])) rc = LGPU_E_NOMEM;
  bool folded = false;
  if (!rc && fold) {
    folded = lazy_run_mix(zs, z2s.data(), n, reinterpret_cast<Dev (*)[3]>(outs.data()), &rc);
    if (!rc && !folded) rc = l2_first();
  }
  if (!rc && !folded && sink) rc = lazy_run_sink(zs, n, reinterpret_cast<Dev (*)[3]>(outs.data()));
  else if (!rc && !folded) {
    std::vector<uint8_t *> outp((size_t)n);
    for (int i = 0; i < n; i++) outp[(size_t)i] = (uint8_t *)outs[(size_t)i * 3].d;
    rc = lazy_run_rgba(zs, n, outp.data());
  }
  if (rc) {                                                                            // the programs stay pending; what was enqueued wrote scratch only
    for (Dev &o : outs) if (o.d) { o.stream = S(); pool_give(o); }
    return rc;
  }
  for (int i = 0; i < n; i++) {
    Lazy *z = zs[i];
    for (int p = 0; p < np; p++) {
      const void *h = sink ? z->sph[p] : hs[i];
      Dev &o = outs[(size_t)i * 3 + p];
      res_update(h, [&o, z](Dev *e) {
        if (!e || e->lazy != z) return;
        const int readers = e->lazy_readers;
        *e = o;
        e->stream = S(); e->nr = 0; e->lazy = nullptr; e->lazy_readers = readers;
        o = Dev();
      });
    }
    if (z->blend && z->l2h)
      res_update(z->l2h, [z, folded](Dev *l2) {
        if (l2) { if (!folded) note_use(*l2, false); if (l2->lazy_readers > 0) l2->lazy_readers--; }      // folded: the entry is still the program, whose source planes lazy_run_mix has marked
        z->l2h = nullptr;
      });
    for (int p = 0; p < np; p++) { Dev &o = outs[(size_t)i * 3 + p]; if (o.d) { o.stream = S(); pool_give(o); o = Dev(); } }          // (the plane vanished meanwhile: cannot happen under the host's own ordering)
    lazy_free(z, true);
  }
  return LGPU_OK;
}
// n pending programs of ONE shape that end in LZ_SINK, into souts[track][plane] (the conversion's Y, U, V order).  The form is chosen by tools/bench_sink_chain.py's
// measurement (profiles/r08/sink_chain.md: 16 x 4K -> 1080p, blend + LUT, the fused launch 157 us against 185 for the two launches to YUV420P, 147 against 187 to
// UYVY, rounds within 2 us of each other): whatever fits lgpu_chain_to_yuv's one-launch form takes it -- ONE launch, no RGBA frame; every other shape runs its RGBA
// stages as the chain group into scratch frames, followed by ONE lgpu_rgb_to_yuv_batch per 16 tracks; a program of the sink stage alone is that batch on the
// resident frames.  SEAM_STAGED: stage by stage and one conversion per track, for tests.  (FLAT_SINK_FORMATS: above lazy_folds, which asks it too.)
static int lazy_run_sink(Lazy *const *zs, int n, Dev (*souts)[3]) {
  const Lazy *z0 = zs[0];
  const bool staged = lgpu_tuning_get("SEAM_STAGED") > 0;
  const bool rgba_stages = z0->yuv || z0->swap || z0->scale || z0->canvas || z0->blend || z0->lut;
  int rc = LGPU_OK;
  const int row_bytes[3] = {z0->sfmt == 4 ? z0->sww : z0->sww * 2, z0->sww >> 1, z0->sww >> 1};
  for (int i = 0; i < n && !rc; i++)
    for (int p = 0; p < z0->snp && !rc; p++)
      if (z0->sors[p] != row_bytes[p]) rc = lgpu_fill(souts[i][p].d, 0, z0->sbytes[p], S());      // the row padding of a fresh plane is zero (calloc in the eager path)
  if (rc) return rc;
  // Which sink formats (2 UYVY, 3 YUYV, 4 4:2:0) a group that starts at YUV planes takes as ONE lgpu_chain_yuv420p_to_yuv launch: those for which
  // tools/bench_transcode_chain.py shows the launch ahead of lgpu_chain_yuv420p + lgpu_rgb_to_yuv_batch by more than the round-to-round spread of the latter.
  // profiles/r09/transcode_chain.md (16 x 4K -> 1080p, blend + LUT, five interleaved rounds): to UYVY 214.3 us against 244.7 for the two launches (spread 0.2 us) --
  // taken, and YUYV with it (the same instantiation); to YUV420P 258.9 us against 243.4 (spread 1.9 us) -- the 4:2:0 form's 98-105 registers hold it to four waves per
  // SIMD -- so 4:2:0 keeps today's two launches.
  const bool transcode_fused = z0->sfmt == 2 || z0->sfmt == 3;
  // lives_gpu_set_flat_yuv(1): an UNSCALED group from YUV planes to a YUV sink as ONE lgpu_chain_flat_yuv420p_to_yuv launch, for the sink formats FLAT_SINK_FORMATS
  // names: those for which tools/bench_flat_chain.py shows the launch ahead of today's three (lgpu_yuv420p_to_rgb_batch, lgpu_chain_amounts, lgpu_rgb_to_yuv_batch) by
  // more than the round-to-round spread of the latter.  profiles/r11/flat_chain.md (16 x 1080p, blend + LUT, five interleaved rounds): to UYVY 157.2 us against 274.2
  // (spread 0.4 us), YUYV with it (the same instantiation); to YUV420P 159.7 us against 271.7 (spread 0.7 us) -- all taken.  (RGBA, lazy_run_rgba: 158.0 against 227.3.)
  const bool flat_sink = FLAT_SINK_FORMATS(z0->sfmt);
  // The one-launch routes: the sink takes the whole frame the chain ends at, and at most one of them has the group's shape.
  //   lgpu_chain_yuv420p_to_yuv                                  4:2:0 planes, scaled, to the formats of transcode_fused
  //   lgpu_chain_flat_yuv420p_to_yuv / lgpu_chain_flat_yuv422    YUV planes that keep their size, to the formats of flat_sink
  //   lgpu_chain_to_yuv                                          an RGBA frame, scaled
  // A shape that the route's entry point refuses takes today's launches below.
  const bool one_launch = !staged && !z0->canvas && z0->sww == z0->w && z0->shh == z0->h && n <= LGPU_CHAIN_MAX_TRACKS;
  const bool via_transcode = one_launch && transcode_fused && z0->yuv && z0->yfmt == 4 && z0->scale;
  const bool via_flat = one_launch && flat_sink && g_flat_yuv.load() && z0->yuv && !z0->scale;
  const bool via_to_yuv = one_launch && z0->scale && !z0->yuv;
  if (via_transcode || via_flat || via_to_yuv) {
    // (the source planes are awaited as in lazy_run_rgba; lazy_run_group gives them back with their reader streams kept)
    for (int i = 0; i < n; i++) lazy_await(zs[i]);
    const lgpu_chain_params pr = lazy_params(z0, true);
    const lgpu_chain_sink sk = lazy_sink(z0);
    const std::vector<uint8_t> amounts = lazy_amounts(zs, n);
    const uint8_t *const blend_amounts = z0->blend ? amounts.data() : nullptr;
    bool done;
    if (via_to_yuv) {
      const std::vector<lgpu_chain_sink_track> tr = lazy_sink_tracks(zs, n, souts);
      done = lazy_route(lgpu_chain_to_yuv(&pr, &sk, tr.data(), n, blend_amounts, S()), RT_SINK, 1, n, &rc);
    } else {
      // from YUV planes to YUV planes: neither RGBA frame exists
      const lgpu_yuv_source ys = lazy_source<lgpu_yuv_source>(z0);
      const std::vector<lgpu_chain_yuv_sink_track> tr = lazy_yuv_sink_tracks(zs, n, nullptr, souts);
      if (via_transcode)           // the call's launches: LGPU_CHAIN_TRANSCODE_TRACKS tracks each
        done = lazy_route(lgpu_chain_yuv420p_to_yuv(&pr, &ys, &sk, tr.data(), n, blend_amounts, S()), RT_YUV | RT_SINK | RT_TRANSCODE,
                          (n + LGPU_CHAIN_TRANSCODE_TRACKS - 1) / LGPU_CHAIN_TRANSCODE_TRACKS, n, &rc);
      else if (z0->yfmt == 4)      // the call's launches: 32 tracks each to YUV420P
        done = lazy_route(lgpu_chain_flat_yuv420p_to_yuv(&pr, &ys, &sk, tr.data(), n, blend_amounts, S()), RT_SINK | RT_FLAT, z0->sfmt == 4 ? (n + 31) / 32 : 1, n, &rc);
      else {
        const lgpu_yuv422_source y4 = lazy_source<lgpu_yuv422_source>(z0);
        done = lazy_route(lgpu_chain_flat_yuv422(&pr, &y4, nullptr, &sk, tr.data(), n, blend_amounts, S()), RT_SINK | RT_FLAT, z0->sfmt == 4 ? (n + 31) / 32 : 1, n, &rc);
      }
    }
    if (done || rc) return rc;
  }
  // the RGBA frames the conversion reads: the programs' results in scratch, or -- a program of the sink stage alone -- the resident frames themselves
  std::vector<const uint8_t *> rgba((size_t)n);
  int rrow = z0->srs;
  void *scr = nullptr;
  if (rgba_stages) {
    const size_t per = ((size_t)z0->rs * z0->h + 63) & ~(size_t)63;
    if ((rc = lgpu_malloc_ordered(&scr, per * (size_t)n + 64, S()))) return rc;
    std::vector<uint8_t *> outp((size_t)n);
    for (int i = 0; i < n; i++) { outp[(size_t)i] = (uint8_t *)scr + (size_t)i * per; rgba[(size_t)i] = outp[(size_t)i]; }
    rc = lazy_run_rgba(zs, n, outp.data());
    rrow = z0->rs;
  } else
    for (int i = 0; i < n; i++) { lazy_await(zs[i]); rgba[(size_t)i] = (const uint8_t *)zs[i]->src.d; }
  int ors[4] = {z0->sors[0], z0->sors[1], z0->sors[2], 0};
  for (int i0 = 0; i0 < n && !rc; i0 += (staged ? 1 : LGPU_FX_MAX_FRAMES)) {
    const int m = staged ? 1 : std::min(n - i0, (int)LGPU_FX_MAX_FRAMES);
    uint8_t *dp[LGPU_FX_MAX_FRAMES * 4];
    memset(dp, 0, sizeof dp);
    for (int i = 0; i < m; i++) for (int p = 0; p < z0->snp; p++) dp[i * 4 + p] = (uint8_t *)souts[i0 + i][p].d;
    if (staged) rc = lgpu_rgb_to_yuv(rgba[(size_t)i0], rrow, z0->sww, z0->shh, z0->sorder, 1, dp, ors, z0->sfmt, 0, z0->swhich, S());
    else rc = lgpu_rgb_to_yuv_batch(rgba.data() + i0, rrow, z0->sww, z0->shh, z0->sorder, 1, dp, ors, z0->sfmt, 0, z0->swhich, m, S());
    if (!rc) { g_lz_sink_launches++; g_lz_sink_tracks += (unsigned long long)m; }
  }
  if (scr) lgpu_free_ordered(scr, S());
  return rc;
}
// the pending program of plane h, if any, runs now (on the calling thread's stream)
bool lazy_materialise(const void *h) {
  std::lock_guard<std::mutex> run(g_lazy_mu);
  Dev e;
  if (!res_peek(h, &e)) return false;
  Lazy *z = e.lazy;
  if (!z) return true;                      // somebody else ran it meanwhile
  return lazy_run_group(&z, &h, 1) == LGPU_OK;
}
// programs that read plane h as their layer 2 run before h changes
void lazy_run_readers_of(const void *h) {
  for (int guard = 0; guard < 64; guard++) {
    const void *reader = nullptr;
    Dev read;
    if (!res_peek(h, &read) || read.lazy_readers <= 0) return;
    res_scan([&](const void *key, Dev &e) {          // (rare: a plane that pending programs read is about to change) look for one of them, shard by shard
      if (!(e.lazy && e.lazy->blend && e.lazy->l2h == h)) return RES_KEEP;
      reader = key;
      return RES_STOP;
    });
    if (!reader) {
      res_update(h, [](Dev *e) { if (e) e->lazy_readers = 0; });
      return;
    }
    if (!lazy_materialise(reader)) return;
  }
}
// The plane of layer l becomes (or stays) the subject of a pending program that can still take `stage`.  Returns the program DETACHED from the table (the caller
// records its stage and registers it under the layer's new host plane with lazy_attach, or puts it back under the old one on failure), or nullptr: not deferrable.
Lazy *lazy_detach(const Layer &l, int stage) {
  if (!g_deferred.load(std::memory_order_relaxed) || !t_pinned || !lazy_pal(l.pal) || l.nplanes != 1 || (l.rs[0] & 3) || ((uintptr_t)l.pd[0] & 3)) return nullptr;
  const size_t n = (size_t)l.rs[0] * l.height;
  for (int pass = 0; pass < 2; pass++) {
    bool need_run = false, taken = false;
    const Dev e = res_take_if(l.pd[0], [&](const Dev &c) {
      if (c.bytes < n) return false;
      if (c.lazy_readers > 0) return false;                                // someone's layer 2: it keeps its pixels
      if (c.lazy && c.lazy->stage >= stage) { need_run = true; return false; }
      return taken = true;
    });
    if (!need_run && !taken) return nullptr;                               // (or not resident at all)
    if (need_run) { if (!lazy_materialise(l.pd[0])) return nullptr; continue; }    // the recorded program cannot take this stage: it runs, a new one starts from its result
    if (e.lazy) return e.lazy;
    Lazy *z = new Lazy;
    z->src = e; z->sw = l.width; z->sh = l.height; z->srs = l.rs[0];
    z->w = l.width; z->h = l.height; z->rs = l.rs[0];
    return z;
  }
  return nullptr;
}
void lazy_attach(const void *h, Lazy *z) {
  Dev e;
  g_lz_recorded++;
  e.lazy = z; e.bytes = (size_t)z->rs * z->h; e.stream = kIdle;
  const Dev old = res_swap(h, e);
  if (old.d || old.lazy) pool_give(old);
}
// put a detached program / plane back under the host plane it came from (a stage could not be recorded after all)
void lazy_reattach(const void *h, Lazy *z) {
  if (z->stage == LZ_NONE) {              // it was an ordinary resident plane
    Dev e = z->src;
    delete z;
    res_swap(h, e);
    return;
  }
  lazy_attach(h, z);
}
// new host plane(s) for the plane a recorded stage produces; the old host plane is released, the program moves under the new pointer
bool lazy_commit(weed_plant_t *layer, const Layer &l, Lazy *z, int pal, int width, int height, int alignment) {
  NewPlanes np;
  if (!alloc_planes(pal, width, height, alignment, &np)) return false;
  z->w = width; z->h = height; z->rs = np.rs[0];
  lazy_attach(np.pd[0], z);
  free_host_planes(l);                    // free_planes without the table (the entry has moved)
  commit_planes(layer, pal, width, height, np);
  return true;
}

// convert_layer_palette_full(YUV420P / YVU420P -> RGBA32 / BGRA32) on a pinned layer whose three planes are resident: recorded as stage LZ_YUV of a new program
// that takes the planes out of the table (owned; external surfaces borrowed) and stands for the new RGBA host plane.  false: not recorded, nothing changed.
// Under lives_gpu_set_flat_yuv(1) ONLY, YUV422P (three planes, full-height chroma) and UYVY / YUYV (one plane whose width leaf counts macropixels: the RGBA frame
// is twice as wide) are recorded the same way; with the switch off these palettes keep the eager conversion and no counter moves.
bool lazy_record_yuv(weed_plant_t *layer, const Layer &l, int outpl, int which, int new_gamma, int flags) {
  const bool p420 = l.pal == WEED_PALETTE_YUV420P || l.pal == WEED_PALETTE_YVU420P, packed = l.pal == WEED_PALETTE_UYVY || l.pal == WEED_PALETTE_YUYV;
  if (!g_deferred.load(std::memory_order_relaxed) || !t_pinned || !lazy_pal(outpl)) return false;
  if (!p420 && !((l.pal == WEED_PALETTE_YUV422P || packed) && g_flat_yuv.load())) return false;
  const int np = packed ? 1 : 3, owidth = packed ? l.width * 2 : l.width;          // macropixels -> pixels (:13010)
  if (l.nplanes != np || owidth < 2 || (owidth & 1)) return false;
  if (packed && ((l.rs[0] & 3) || l.rs[0] < owidth * 2)) return false;            // rows that are not 4-byte aligned or too short: the one launch refuses them (and so does the batched fallback), so nothing is recorded and the eager call answers
  const int iu = packed ? 0 : (l.pal == WEED_PALETTE_YVU420P) ? 2 : 1, iv = packed ? 0 : 3 - iu;            // swap_chroma_planes (:12353)
  const int ch = packed ? 0 : plane_h(l, 1);
  const void *hp[3] = {l.pd[0], l.pd[iu], l.pd[iv]};
  const size_t need[3] = {(size_t)l.rs[0] * l.height, (size_t)l.rs[iu] * ch, (size_t)l.rs[iv] * ch};
  for (int p = 0; p < np; p++) {
    Dev e;
    if (!res_peek(hp[p], &e) || !e.d || e.lazy || e.bytes < need[p] || e.lazy_readers > 0) return false;
  }
  Dev d[3];
  for (int p = 0; p < np; p++) d[p] = res_take(hp[p]);
  auto put_back = [&]() {
    for (int p = 0; p < np; p++) if (d[p].d) res_swap(hp[p], d[p]);
  };
  if (!d[0].d || (!packed && (!d[1].d || !d[2].d))) { put_back(); return false; }
  Lazy *z = new Lazy;
  z->src = d[0]; z->yu = d[1]; z->yv = d[2]; z->yuv = true; z->stage = LZ_YUV;
  z->yfmt = p420 ? 4 : l.pal == WEED_PALETTE_YUV422P ? 5 : l.pal == WEED_PALETTE_UYVY ? 2 : 3;
  z->sw = owidth; z->sh = l.height; z->srs = owidth * 4;
  z->ystr[0] = l.rs[0]; z->ystr[1] = packed ? 0 : l.rs[iu]; z->ystr[2] = packed ? 0 : l.rs[iv]; z->usz = packed ? 0 : (long)need[1]; z->vsz = packed ? 0 : (long)need[2];
  z->order = pal_red_first(outpl) ? 0 : 1; z->which = packed ? (which & 1) : which; z->quality = g_prefs.pb_quality;      // K3 takes the YCbCr tables only
  if (!lazy_commit(layer, l, z, outpl, owidth, l.height, 0)) { delete z; put_back(); return false; }
  g_lz_yuv_recorded++;
  if (new_gamma != l.gamma) set_int(layer, WEED_LEAF_GAMMA_TYPE, new_gamma);
  if (flags != l.flags) set_int(layer, kLeafHostFlags, flags);
  delete_yuv_leaves(layer);
  return true;
}

}  // namespace seam
#pragma GCC visibility pop
using namespace seam;

extern "C" {
// deferred execution (see "deferred execution on pinned layers" above): on (default) / off; returns the previous setting
int lives_gpu_set_deferred(int on) { return g_deferred.exchange(on ? 1 : 0); }
// unscaled YUV groups as one launch (flat.hip): off (default) / on; returns the previous setting
int lives_gpu_set_flat_yuv(int on) { return g_flat_yuv.exchange(on ? 1 : 0); }
// a blend's second layer may stay pending: 0 off (default: a blend runs a pending layer 2 when it is recorded), 1 on and a flush folds the pairs MIX_FOLD_PAIRS
// names, 2 on and it folds every pair the one-launch forms take, 3 on and it never folds (the layer-2 programs run as a group ahead of their readers); returns the
// previous mode.  Another number is taken as 0
int lives_gpu_set_pending_layer2(int mode) { return g_pending_l2.exchange(mode >= 1 && mode <= 3 ? mode : 0); }
// counters since the library was loaded: [0] stages recorded, [1] fused chain launches made for pending programs, [2] tracks (programs) those launches carried,
// [3] programs run stage by stage (shapes the fused kernel does not take)
void lives_gpu_deferred_stats(unsigned long long out[4]) {
  if (!out) return;
  out[0] = g_lz_recorded.load(); out[1] = g_lz_chain_launches.load(); out[2] = g_lz_chain_tracks.load(); out[3] = g_lz_staged.load();
}
// the same counters, then [4] YUV420P / YVU420P conversions recorded, [5] one-launch YUV chain launches (lgpu_chain_yuv420p) and [6] the tracks they carried,
// [7] conversion pre-launches of the two-launch path (lgpu_yuv420p_to_rgb_batch), [8] sink conversions recorded (LZ_SINK), [9] sink launches (a fused
// lgpu_chain_to_yuv launch, also counted in [1], or one lgpu_rgb_to_yuv_batch / lgpu_rgb_to_yuv) and [10] the tracks they carried, [11] those of [9] that were fused lgpu_chain_to_yuv launches (the others converted an
// RGBA frame), [12] launches that ran from YUV planes to YUV planes (lgpu_chain_yuv420p_to_yuv; each is also counted in [1], [5], [9] and [11]), [13] launches of the
// unscaled one-launch forms (lives_gpu_set_flat_yuv: lgpu_chain_flat_yuv420p, counted in [1] too, and lgpu_chain_flat_yuv420p_to_yuv, counted in [1], [9] and [11] too;
// lgpu_chain_flat_yuv422 from YUV422P / UYVY / YUYV layers as whichever of the two it stands for, such layers' recorded conversions in [4], their batched fallback in [7]) and
// [14] the tracks they carried; lives_gpu_set_pending_layer2: [15] blends recorded against a pending layer 2, [16] mix launches (lgpu_chain_flat_yuv_mix[_canvas]: each is
// also counted in [1] and [13], and with a sink in [9] and [11]) and [17] the tracks they carried, [18] layer-2 programs run ahead of their readers; at most n entries are
// written (19 exist; a caller that passes n <= 15 sees what it saw before)
void lives_gpu_deferred_stats_n(unsigned long long *out, int n) {
  if (!out || n <= 0) return;
  const unsigned long long v[19] = {g_lz_recorded.load(), g_lz_chain_launches.load(), g_lz_chain_tracks.load(), g_lz_staged.load(),
                                    g_lz_yuv_recorded.load(), g_lz_yuv_launches.load(), g_lz_yuv_tracks.load(), g_lz_yuv_pre.load(),
                                    g_lz_sink_recorded.load(), g_lz_sink_launches.load(), g_lz_sink_tracks.load(), g_lz_sink_fused.load(),
                                    g_lz_transcode.load(), g_lz_flat_launches.load(), g_lz_flat_tracks.load(),
                                    g_lz_l2_recorded.load(), g_lz_mix_launches.load(), g_lz_mix_tracks.load(), g_lz_l2_first.load()};
  for (int i = 0; i < n && i < 19; i++) out[i] = v[i];
}
// Run the pending programs of these layers now, on the calling thread's stream: programs of equal shape (the tracks of one plan step) share ONE launch of the
// fused chain kernel.  The layers stay pinned, nothing is downloaded, the host does not wait.  What a host calls once per tick when the plan steps of its tracks
// have returned (src/nodemodel.c:2027-2101 runs them on pool threads and collects them); without it every program still runs, by itself, when its pixels are needed.
int lives_gpu_layers_flush(lives_gpu_layer_t *const *layers, int nlayers) {
  if (!ready() || (nlayers > 0 && !layers)) return LGPU_E_BADARG;
  std::vector<const void *> hs;
  for (int i = 0; i < nlayers; i++) {
    Layer l;
    if (!layers[i] || !read_layer(layers[i], &l)) continue;
    for (int p = 0; p < l.nplanes; p++) hs.push_back(l.pd[p]);
  }
  std::lock_guard<std::mutex> run(g_lazy_mu);
  // every pending program ONCE, under the first of its planes listed: a program that ends in LZ_SINK is registered under up to three host planes, and a layer may
  // be listed twice.  Running a group deletes its programs, so no pointer may be looked at again after its group has run.
  std::vector<Lazy *> zs;
  std::vector<const void *> zh;
  {
    std::unordered_set<const Lazy *> seen;
    for (size_t i = 0; i < hs.size(); i++) {
      Dev e;
      Lazy *z = res_peek(hs[i], &e) ? e.lazy : nullptr;
      if (z && seen.insert(z).second) { zs.push_back(z); zh.push_back(hs[i]); }
    }
  }
  int rc = LGPU_OK;
  std::vector<char> done(zs.size(), 0);
  // a listed program that is the pending layer 2 of a listed program is not a group member of its own: its readers' group folds it into its launch -- it then
  // STAYS pending -- or runs it ahead of them (lazy_run_group), as it does for a layer 2 that is not listed at all
  for (size_t i = 0; i < zs.size(); i++)
    if (Lazy *z2 = lazy_l2_program(zs[i]))
      for (size_t k = 0; k < zs.size(); k++) if (zs[k] == z2) done[k] = 1;
  for (size_t i = 0; i < zs.size(); i++) {
    if (done[i]) continue;
    std::vector<Lazy *> gz;
    std::vector<const void *> gh;
    for (size_t k = i; k < zs.size() && (int)gz.size() < LGPU_CHAIN_MAX_TRACKS; k++)
      if (!done[k] && lazy_same_shape(zs[i], zs[k])) { done[k] = 1; gz.push_back(zs[k]); gh.push_back(zh[k]); }
    const int r = lazy_run_group(gz.data(), gh.data(), (int)gz.size());
    if (r && !rc) rc = r;
  }
  return rc;
}
// livesgpu_fx.so's "chroma blend" on a plane that is a pending program (in place: out channel = in channel 0): the blend with layer 2 is recorded as the program's
// next stage.  1 = recorded, the effect has nothing left to do; 0 = not applicable, the effect runs its kernel (acquiring the planes runs what is pending).
int lives_gpu_deferred_blend_chroma(const void *dst_host, int orow, int width, int height, int palette, const void *layer2_host, int irow2, int bf) {
  if (!g_deferred.load(std::memory_order_relaxed) || !dst_host || !layer2_host || dst_host == layer2_host || !lazy_pal(palette) || (irow2 & 3) || !ready()) return 0;
  const bool takes_it = res_update(dst_host, [&](Dev *e) {
    if (!e || !e->lazy || e->lazy_readers > 0) return false;
    const Lazy *z = e->lazy;
    return !(z->stage >= LZ_BLEND || z->w != width || z->h != height || z->rs != orow);
  });
  if (!takes_it) return 0;
  // lives_gpu_set_pending_layer2: a layer 2 that is itself a pending program of this size, with no blend and no sink of its own, is NOT run: it becomes a plane a
  // pending program reads as it stands, and whoever runs the reader resolves it (lazy_l2_program)
  if (g_pending_l2.load()) {
    const bool pending = res_update(layer2_host, [&](Dev *l2) {
      if (!l2 || !l2->lazy) return false;
      const Lazy *z2 = l2->lazy;
      if (z2->blend || z2->sink || z2->w != width || z2->h != height || z2->rs != irow2) return false;
      l2->lazy_readers++;
      return true;
    });
    if (pending) {
      const bool taken = res_update(dst_host, [&](Dev *e) {
        if (!(e && e->lazy && e->lazy->stage < LZ_BLEND)) return false;
        Lazy *z = e->lazy;
        g_lz_recorded++;
        z->blend = true; z->bf = bf & 0xFF; z->l2h = layer2_host; z->l2 = Dev(); z->l2pend = true; z->l2rs = irow2; z->stage = LZ_BLEND;
        return true;
      });
      if (!taken) {
        res_update(layer2_host, [](Dev *l2) { if (l2 && l2->lazy_readers > 0) l2->lazy_readers--; });
        return 0;
      }
      g_lz_l2_recorded++;
      return 1;
    }
  }
  const size_t n2 = (size_t)irow2 * height;
  uint8_t *l2d = acquire(layer2_host, n2, false);          // layer 2 itself may be pending: it runs; this thread's stream is behind its writer
  if (!l2d) return 0;
  // layer 2 first (its own shard): it becomes a plane a pending program reads; then the program takes the stage -- or, should the plane have changed hands in
  // between (it cannot under the host's own ordering), layer 2 is let go again
  Dev l2copy;
  const bool read = res_update(layer2_host, [&](Dev *l2) {
    if (!l2 || !l2->d) return false;
    l2copy = *l2;
    l2->lazy_readers++;
    return true;
  });
  if (!read) return 0;
  const bool taken = res_update(dst_host, [&](Dev *e) {
    if (!(e && e->lazy && e->lazy->stage < LZ_BLEND)) return false;
    Lazy *z = e->lazy;
    g_lz_recorded++;
    z->blend = true; z->bf = bf & 0xFF; z->l2h = layer2_host; z->l2 = l2copy; z->l2rs = irow2; z->stage = LZ_BLEND;
    return true;
  });
  if (!taken) {
    res_update(layer2_host, [](Dev *l2) { if (l2 && l2->lazy_readers > 0) l2->lazy_readers--; });
    return 0;
  }
  return 1;
}
}  // extern "C"
