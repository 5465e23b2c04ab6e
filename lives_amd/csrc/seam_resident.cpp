// seam_resident.cpp -- device residency of pinned layers (seam_resident.h): the per-thread streams and their hand-over, the residency table's shards, the pool
// of device buffers, the per-thread scratch and the data movement of one seam call (struct Work), and the public entry points that are about nothing else:
// lives_gpu_layer_pin / _pin_device / _copy / _sync / _unpin / _forget, lives_gpu_pinned_calloc / _free, lives_gpu_resident_lookup / _acquire / _release,
// lives_gpu_thread_stream, lives_gpu_stream_follow, lives_gpu_transfer_stats.
#include <stdint.h>
#include <string.h>
#include <utility>
#include <vector>
#include "seam_resident.h"
#include "seam_lazy.h"

#pragma GCC visibility push(hidden)
namespace seam {

// Streams: every host thread enqueues on a stream of its own (LiVES runs plan steps and conversions on pool threads, src/threading.c; one shared
// stream would run the small kernels of different tracks one after the other).  Non-blocking streams: a launch on a blocking one costs twice the host
// time (ordering against the null stream is checked per launch).  livesgpu_fx.so enqueues on the same per-thread streams (lives_gpu_resident_acquire /
// _release); a caller on the null stream is ordered at its hand-over (lives_gpu_resident_lookup) like any other stream.  Never destroyed (a thread_local destructor of the main thread runs after HIP's teardown), but recycled:
// A thread that ends hands its stream (and its hand-over event) to a spare list, and a new thread takes one from there before it creates one: a host that
// runs short-lived threads does not pile up streams.  No HIP call in the destructor (it may run after HIP's teardown); the list itself is never destroyed.
struct SpareGpuObjects { std::atomic<bool> held{false}; std::vector<void *> streams, events; };
static SpareGpuObjects &spares() { static SpareGpuObjects *p = new SpareGpuObjects; return *p; }
struct ThreadGpu {
  bool armed = false;                             // the thread's stream and event themselves are plain data (t_ts, seam_resident.h)
  ~ThreadGpu() {
    void *const stream = t_ts.stream, *const event = t_ts.event;
    if (!stream && !event) return;
    SpareGpuObjects &sp = spares();
    while (sp.held.exchange(true, std::memory_order_acquire)) sched_yield();
    if (stream) sp.streams.push_back(stream);
    if (event) sp.events.push_back(event);
    sp.held.store(false, std::memory_order_release);
  }
};
static thread_local ThreadGpu t_gpu;
__thread ThreadStream t_ts = {nullptr, nullptr, false};
void *first_stream() {
  if (!t_ts.tried) {
    t_ts.tried = true;
    t_gpu.armed = true;                           // (constructs it: its destructor runs when this thread ends)
    SpareGpuObjects &sp = spares();
    while (sp.held.exchange(true, std::memory_order_acquire)) sched_yield();
    if (!sp.streams.empty()) { t_ts.stream = sp.streams.back(); sp.streams.pop_back(); }
    if (!sp.events.empty()) { t_ts.event = sp.events.back(); sp.events.pop_back(); }
    sp.held.store(false, std::memory_order_release);
    if (!t_ts.stream && lgpu_stream_create(&t_ts.stream, 1) != LGPU_OK) t_ts.stream = nullptr;     // the null stream then: everything is ordered, nothing overlaps
  }
  return t_ts.stream;
}
#define t_event (t_ts.event)

char g_idle_tag;
ResShard g_shards[kResShards];
static SpinLock g_pool_mu;                               // guards g_pool
static std::atomic<unsigned long long> g_h2d{0}, g_d2h{0};   // PCIe byte counters (tests check the residency contract with them)
__thread bool t_pinned = false;             // the call in progress works on a pinned layer
// t_ts.event: this thread's hand-over event (re-recorded at every hand-over; a wait holds the record it saw)

void follow_other(void *other) {                  // (follow, seam_resident.h: other is neither this thread's stream nor kIdle)
  if (!t_event && lgpu_event_create(&t_event) != LGPU_OK) t_event = nullptr;
  if (t_event && lgpu_event_record(t_event, other) == LGPU_OK && lgpu_stream_wait_event(S(), t_event) == LGPU_OK) return;
  lgpu_sync(other);                               // no event to be had: wait for that stream on the host instead
}

// Device buffers of resident planes: a pinned layer going through a chain of seam calls takes a new plane per call and drops the old one, and neither
// side may wait for the device.  First level: a list of dropped buffers (a hit costs nothing).  Behind it the device's stream-ordered pool
// (lgpu_malloc_ordered: hipMallocAsync / hipFreeAsync on the calling thread's stream; ~10 us each, no synchronisation -- hipMalloc costs ~0.1 ms
// and hipFree waits for the device to drain, tools/alloc_probe.hip).  A buffer from the list carries the stream of its last use; a taker on another
// stream waits for that one.
// Buffers come in size classes ({1, 1.25, 1.5, 1.75} x 2^k, at least 64 KB): planes of similar size -- a 960 x 540 frame and its 960 x 600 letterboxed
// canvas -- recycle each other's buffers instead of each going to the device pool.  The list keeps up to 8 GB (a 288 GB device; what a few dozen 4K
// layers in flight hand back and forth) and is bucketed by class, so in steady state no call reaches hipMallocAsync / hipFreeAsync at all: under
// sixteen host threads those two were where the seam calls queued (tools/bench_seam_mt.py).
static std::unordered_map<size_t, std::vector<Dev>> g_pool;
static size_t g_pool_bytes = 0;
constexpr size_t kPoolMaxBytes = 8ull << 30;
static size_t pool_class(size_t n) {
  if (n <= (64u << 10)) return 64u << 10;
  size_t base = 64u << 10;
  while (base * 2 <= n) base *= 2;
  const size_t step = base / 4;
  return base + (n - base + step - 1) / step * step;
}
bool pool_take(size_t n, Dev *out) {
  const size_t cls = pool_class(n + 64);
  bool hit = false;
  {
    std::lock_guard<SpinLock> lk(g_pool_mu);
    auto it = g_pool.find(cls);
    if (it != g_pool.end() && !it->second.empty()) {
      std::vector<Dev> &v = it->second;
      int best = (int)v.size() - 1;                                // newest first; one whose last use needs no cross-stream wait if there is one near the top
      for (int i = best, k = 0; i >= 0 && k < 8; i--, k++)
        if ((v[i].stream == S() || v[i].stream == kIdle) && v[i].nr == 0) { best = i; break; }
      *out = v[best];
      v[best] = v.back();
      v.pop_back();
      g_pool_bytes -= cls;
      hit = true;
    }
  }
  if (hit) { await(*out); out->stream = S(); out->nr = 0; return true; }
  Dev b;
  if (lgpu_malloc_ordered(&b.d, cls, S()) != LGPU_OK) return false;
  b.bytes = cls; b.stream = S();
  *out = b;
  return true;
}
void pool_give(Dev b) {
  if (b.lazy) { lazy_discard(b.lazy); return; }       // a pending program nobody will ever look at: its source frame goes back, nothing runs
  if (!b.d || b.external) return;
  {
    std::lock_guard<SpinLock> lk(g_pool_mu);
    if (g_pool_bytes + b.bytes <= kPoolMaxBytes) {
      g_pool[b.bytes].push_back(b);
      g_pool_bytes += b.bytes;
      return;
    }
  }
  await(b);                                       // the free is ordered on this thread's stream, which first waits for the last use
  lgpu_free_ordered(b.d, S());
}
// the resident copy registered under host plane h becomes b (last used on the calling thread's stream); whatever was there goes back to the pool
void res_put(const void *h, Dev b) {
  b.stream = S(); b.nr = 0;
  lazy_run_readers_of(h);
  pool_give(res_swap(h, b));
}

void res_drop(const void *h) {
  lazy_run_readers_of(h);
  pool_give(res_take(h));
}
// every resident plane whose host pointer lies inside [base, base + bytes): a contiguous planar block is freed through its base pointer, but its planes 1..3
// are registered under interior pointers and must not survive it (a later block at the same address would otherwise inherit their device copies)
void res_drop_range(const void *base, size_t bytes) {
  std::vector<Dev> gone;
  {
    std::vector<const void *> read;
    res_scan([&](const void *h, Dev &e) {
      if ((uintptr_t)h >= (uintptr_t)base && (uintptr_t)h < (uintptr_t)base + bytes && e.lazy_readers > 0) read.push_back(h);
      return RES_KEEP;
    });
    for (const void *h : read) lazy_run_readers_of(h);
  }
  res_scan([&](const void *key, Dev &e) {
    const uintptr_t h = (uintptr_t)key;
    if (h < (uintptr_t)base || h >= (uintptr_t)base + bytes) return RES_KEEP;
    gone.push_back(e);
    return RES_ERASE;
  });
  for (size_t i = 0; i < gone.size(); i++) {
    bool seen = false;                  // the planes of one sink program share its Lazy: discarded once
    for (size_t k = 0; k < i && gone[i].lazy; k++) seen = seen || gone[k].lazy == gone[i].lazy;
    if (!seen) pool_give(gone[i]);
  }
}
void free_planes(const Layer &l) {
  for (int i = 0; i < l.nplanes; i++) res_drop(l.pd[i]);
  free_host_planes(l);
}

// ---- device scratch (per calling thread; grown on demand) ------------------------------------------------------------
// A thread that ends leaves its buffers on a spare list (no HIP call in a thread_local destructor: the main thread's runs after HIP's teardown) and the next
// new thread starts from them.
struct ScratchSet { void *p[8]; size_t cap[8]; void *stream; };      // stream: where the thread that owned the set enqueued its last use
struct SpareScratch { std::mutex mu; std::vector<ScratchSet> sets; };
static SpareScratch &spare_scratch() { static SpareScratch *sp = new SpareScratch; return *sp; }
struct Scratch {
  void *p[8] = {nullptr};
  size_t cap[8] = {0};
  bool adopted = false;
  void *last_stream = nullptr;
  uint8_t *get(int i, size_t bytes) {
    if (!adopted) {
      adopted = true;
      void *prev = kIdle;
      {
        SpareScratch &sp = spare_scratch();
        std::lock_guard<std::mutex> lk(sp.mu);
        if (!sp.sets.empty()) {
          for (int k = 0; k < 8; k++) { p[k] = sp.sets.back().p[k]; cap[k] = sp.sets.back().cap[k]; }
          prev = sp.sets.back().stream;
          sp.sets.pop_back();
        }
      }
      // the set's previous owner never synchronised on a pinned layer: its last kernels may still read these buffers on ITS stream, which some third thread may
      // have adopted meanwhile -- this thread's stream orders itself behind that stream once, at adoption
      follow(prev);
    }
    last_stream = S();
    if (cap[i] < bytes) {
      if (p[i]) lgpu_free(p[i]);
      p[i] = nullptr; cap[i] = 0;
      if (lgpu_malloc(&p[i], bytes + 64) != LGPU_OK) return nullptr;
      cap[i] = bytes;
    }
    return (uint8_t *)p[i];
  }
  ~Scratch() {
    bool any = false;
    for (int k = 0; k < 8; k++) any = any || p[k];
    if (!any) return;
    SpareScratch &sp = spare_scratch();
    std::lock_guard<std::mutex> lk(sp.mu);
    ScratchSet st;
    for (int k = 0; k < 8; k++) { st.p[k] = p[k]; st.cap[k] = cap[k]; }
    st.stream = last_stream;
    sp.sets.push_back(st);
  }
};
static thread_local Scratch t_scr;

// resident device copy of a plane of the layer the call in progress works on (only pinned layers have one: the table is
// keyed by host pointer, and a host pointer proves nothing about a layer that was never pinned), ready for work on the calling
// thread's stream.  The caller marks the plane (touch_done) once its work is enqueued.
uint8_t *acquire(const void *h, size_t n, bool write) {
  Dev b;
  for (int pass = 0;; pass++) {
    if (!res_peek(h, &b) || b.bytes < n) return nullptr;
    if (!b.lazy && !(write && b.lazy_readers > 0)) break;
    if (pass > 3) return nullptr;
    if (b.lazy && !lazy_materialise(h)) return nullptr;       // whoever needs the pixels themselves gets them: the pending program runs now, on this thread's stream
    if (write && b.lazy_readers > 0) lazy_run_readers_of(h);    // programs that still read this plane see it as it is now
  }
  await(b, write);
  return (uint8_t *)b.d;
}
uint8_t *resident(const void *h, size_t n, bool write) {
  if (!t_pinned || !h) return nullptr;
  return acquire(h, n, write);
}
void touch_done(const void *h, bool write) {
  res_update(h, [&](Dev *e) { if (e) note_use(*e, write); });
}

uint8_t *Work::use(const void *h, size_t n, bool write) {
  uint8_t *r = resident(h, n, write);
  if (r && ntouched < 12) { touched[ntouched] = h; twrite[ntouched++] = write; }
  else if (r) { touch_done(h, true); }                      // cannot happen with <= 4 planes in and out; marked early (as a write) rather than lost
  return r;
}
const uint8_t *Work::in(const uint8_t *h, size_t n, int slot) {
  if (!ok) return nullptr;
  if (uint8_t *r = use(h, n, false)) return r;
  uint8_t *d = t_scr.get(slot, n);
  g_h2d += n;
  ok = d && lgpu_upload(d, h, n, S()) == LGPU_OK;
  return ok ? d : nullptr;
}
// zero: the kernel does not write every byte (row padding, skipped alpha bytes): start from the zeros of the fresh host plane
uint8_t *Work::out(uint8_t *h, size_t n, int slot, bool zero) {
  if (!ok || nout >= 8) { ok = false; return nullptr; }
  Out o;
  o.host = h; o.n = n; o.pooled = false;
  if (t_pinned) {
    if (!pool_take(n, &o.b)) { ok = false; return nullptr; }
    o.pooled = true;
  } else o.b.d = t_scr.get(slot, n);
  ok = o.b.d && (!zero || lgpu_fill(o.b.d, 0, n, S()) == LGPU_OK);
  if (o.b.d) outs[nout++] = o;
  return ok ? (uint8_t *)o.b.d : nullptr;
}
uint8_t *Work::inout(uint8_t *h, size_t n, int slot) {
  if (!ok || nout >= 8) { ok = false; return nullptr; }
  if (uint8_t *r = use(h, n, true)) return r;              // modified where it lives
  uint8_t *d = const_cast<uint8_t *>(in(h, n, slot));
  if (d) { Out o; o.host = h; o.b.d = d; o.n = n; o.pooled = false; outs[nout++] = o; }
  return d;
}
void Work::mark_touched() {
  for (int i = 0; i < ntouched; i++) touch_done(touched[i], twrite[i]);
  ntouched = 0;
}
bool Work::finish() {
  if (!ok) return false;
  bool moved = false;
  for (int i = 0; i < nout && ok; i++) {
    Out &o = outs[i];
    if (o.pooled) {                                         // the buffer becomes the resident copy of the new host plane
      res_put(o.host, o.b);
      o.b = Dev();
    } else {
      g_d2h += o.n;
      ok = lgpu_download(o.host, o.b.d, o.n, S()) == LGPU_OK;
      moved = true;
    }
  }
  mark_touched();
  if (ok && moved) ok = sync();
  done = ok;
  return ok;
}
Work::~Work() {
  if (done) return;
  mark_touched();
  for (int i = 0; i < nout; i++)
    if (outs[i].pooled && outs[i].b.d) { outs[i].b.stream = S(); outs[i].b.nr = 0; pool_give(outs[i].b); }
}

// A call that this library does not serve returns FALSE and the caller's CPU body takes over.  The host bytes of a
// pinned layer are stale by contract, so a pinned layer is first brought home and unpinned: the CPU body then sees the current
// pixels, and no stale device copy survives it.
lives_gpu_boolean decline(weed_plant_t *layer) {
  if (t_pinned && layer) lives_gpu_layer_unpin_impl(layer);
  return 0;
}

// a pinned layer's LUT16 (create_gamma_lut, 65536 x uint16) per (device, from, to, screen gamma): built once, not per frame.  Entries are never evicted -- a
// pointer handed to one host thread may not yet be in a launch when another thread asks for a seventeenth table -- and there are few of them: the gamma pairs
// LiVES uses times the screen gammas a session sets, 128 KB each (a cap of 256 entries = 32 MB is a failure, not an eviction).
struct Lut16Key { int dev, from, to; double screen; bool operator==(const Lut16Key &o) const { return dev == o.dev && from == o.from && to == o.to && screen == o.screen; } };
std::mutex g_l16_mu;
std::vector<std::pair<Lut16Key, void *>> g_l16;
const uint16_t *device_lut16(int from, int to) {
  const Lut16Key k = {g_prefs.device, from, to, g_prefs.screen_gamma};
  std::lock_guard<std::mutex> lk(g_l16_mu);
  for (auto &e : g_l16) if (e.first == k) return (const uint16_t *)e.second;
  if (g_l16.size() >= 256) return nullptr;
  std::vector<uint16_t> h(65536);
  if (!lgpu_gamma_lut16(1.0, from, to, g_prefs.screen_gamma, h.data())) return nullptr;
  void *d = nullptr;
  if (lgpu_malloc(&d, 65536 * 2) != LGPU_OK) return nullptr;
  if (lgpu_upload(d, h.data(), 65536 * 2, S()) != LGPU_OK || lgpu_sync(S()) != LGPU_OK) { lgpu_free(d); return nullptr; }     // the calling thread's stream; complete before the pointer is shared
  g_l16.push_back({k, d});
  return (const uint16_t *)d;
}

// ---- device residency API (seam 2) ---------------------------------------------------------------------------
static size_t plane_bytes(const Layer &l, int p) { return (size_t)l.rs[p] * plane_rows(l.pal, l.height, p); }
// this thread's stream has just been synchronised: planes whose last use was enqueued on it have no work pending, whoever touches them next need not wait
static void settle(const Layer &l) {
  for (int p = 0; p < l.nplanes; p++) {
    res_update(l.pd[p], [](Dev *e) {
      if (!e) return;
      if (e->stream == S()) e->stream = kIdle;
      int k = 0;
      for (int i = 0; i < e->nr; i++) if (e->rs[i] != S()) e->rs[k++] = e->rs[i];
      e->nr = k;
    });
  }
}
}  // namespace seam
#pragma GCC visibility pop
using namespace seam;

extern "C" {
int lives_gpu_layer_pin(lives_gpu_layer_t *layer) {
  Layer l;
  if (!ready() || !read_layer(layer, &l)) return LGPU_E_BADARG;
  if (has_leaf(layer, kLeafResident)) return LGPU_OK;
  for (int p = 0; p < l.nplanes; p++) {
    const size_t n = plane_bytes(l, p);
    Dev b;
    if (!pool_take(n, &b)) { for (int q = 0; q < p; q++) res_drop(l.pd[q]); return LGPU_E_NOMEM; }
    g_h2d += n;
    if (lgpu_upload(b.d, l.pd[p], n, S()) != LGPU_OK) {
      pool_give(b);
      for (int q = 0; q < p; q++) res_drop(l.pd[q]);
      return LGPU_E_HIP;
    }
    res_put(l.pd[p], b);
  }
  if (!sync()) return LGPU_E_HIP;             // the host may change or free its bytes once pin returns
  settle(l);
  set_int(layer, kLeafResident, 1);
  return LGPU_OK;
}
// A layer whose planes ALREADY are in device memory the caller owns (a hardware decoder's output surfaces, the frame a previous pass left in HBM): the layer is
// pinned with those buffers as its resident planes -- no upload, no copy.  The library reads them where they lie (in-place calls write them) and never frees them;
// they must stay valid until the layer's pixel_data has been replaced by a seam call, or the layer is synchronised / unpinned / forgotten.  producer_stream: the
// stream their contents were produced on (NULL = the null stream; pass lives_gpu_thread_stream() or any stream already synchronised for "complete").
int lives_gpu_layer_pin_device(lives_gpu_layer_t *layer, const void *const *planes_d, int nplanes, void *producer_stream, int producer_done) {
  Layer l;
  if (!ready() || !read_layer(layer, &l) || !planes_d || nplanes != l.nplanes) return LGPU_E_BADARG;
  if (has_leaf(layer, kLeafResident)) return LGPU_E_BADARG;
  for (int p = 0; p < l.nplanes; p++) if (!planes_d[p]) return LGPU_E_BADARG;
  for (int p = 0; p < l.nplanes; p++) {
    Dev b;
    b.d = const_cast<void *>(planes_d[p]); b.bytes = plane_bytes(l, p); b.external = true;
    b.stream = producer_done ? kIdle : producer_stream;
    lazy_run_readers_of(l.pd[p]);
    const Dev old = res_swap(l.pd[p], b);
    if (old.d || old.lazy) pool_give(old);
  }
  set_int(layer, kLeafResident, 1);
  return LGPU_OK;
}
// weed_layer_copy(NULL, slayer) -- the deep copy (src/layers.c:755-846: a new layer, copy_pixel_data_slice) -- copies HOST bytes, which are stale while slayer is
// pinned.  Called on its result, this gives the copy the pixels: dlayer (the same palette, size and rowstrides, host planes of its own) becomes a pinned layer whose
// device planes are device-to-device copies of slayer's (a pending program of slayer runs first); no byte crosses PCIe.  slayer not pinned: nothing to do.
int lives_gpu_layer_copy(lives_gpu_layer_t *dlayer, lives_gpu_layer_t *slayer) {
  Layer s, d;
  if (!ready() || !read_layer(slayer, &s) || !read_layer(dlayer, &d)) return LGPU_E_BADARG;
  if (!has_leaf(slayer, kLeafResident)) return LGPU_OK;
  if (has_leaf(dlayer, kLeafResident) || s.nplanes != d.nplanes || s.pal != d.pal || s.width != d.width || s.height != d.height) return LGPU_E_BADARG;
  for (int p = 0; p < s.nplanes; p++)
    if (s.rs[p] != d.rs[p] || plane_bytes(s, p) != plane_bytes(d, p) || s.pd[p] == d.pd[p]) return LGPU_E_BADARG;      // (a shallow copy shares the planes and their device copies already)
  for (int p = 0; p < s.nplanes; p++) {
    const size_t n = plane_bytes(s, p);
    const uint8_t *src = acquire(s.pd[p], n, false);
    Dev b;
    if (!src || !pool_take(n, &b)) { for (int q = 0; q < p; q++) res_drop(d.pd[q]); return src ? LGPU_E_NOMEM : LGPU_E_BADARG; }
    if (lgpu_copy(b.d, src, n, S()) != LGPU_OK) { pool_give(b); for (int q = 0; q < p; q++) res_drop(d.pd[q]); return LGPU_E_HIP; }
    touch_done(s.pd[p], false);
    b.stream = S();
    res_put(d.pd[p], b);
  }
  set_int(dlayer, kLeafResident, 1);
  return LGPU_OK;
}
int lives_gpu_layer_sync(lives_gpu_layer_t *layer) {
  Layer l;
  if (!ready() || !read_layer(layer, &l)) return LGPU_E_BADARG;
  if (!has_leaf(layer, kLeafResident)) return LGPU_OK;          // never pinned: the host bytes are the planes
  for (int p = 0; p < l.nplanes; p++) {
    const size_t n = plane_bytes(l, p);
    Dev b;
    if (plane_is_lazy(l.pd[p]) && !lazy_materialise(l.pd[p])) return LGPU_E_HIP;        // a pending program runs now
    res_update(l.pd[p], [&](Dev *e) { if (e && e->bytes >= n) { b = *e; note_use(*e, false); } });
    if (!b.d) continue;                                 // this plane's host bytes are current
    await(b, false);                                    // behind the work of whichever thread wrote it last
    g_d2h += n;
    if (lgpu_download(l.pd[p], b.d, n, S()) != LGPU_OK) return LGPU_E_HIP;
  }
  if (!sync()) return LGPU_E_HIP;
  settle(l);
  return LGPU_OK;
}
}  // extern "C"
#pragma GCC visibility push(hidden)
namespace seam {
int lives_gpu_layer_unpin_impl(weed_plant_t *layer) {
  const int rc = lives_gpu_layer_sync(layer);
  Layer l;
  if (read_layer(layer, &l)) for (int p = 0; p < l.nplanes; p++) res_drop(l.pd[p]);
  if (bound() && layer) g_api.leaf_delete(layer, kLeafResident);
  return rc;
}
}  // namespace seam
#pragma GCC visibility pop
extern "C" {
int lives_gpu_layer_unpin(lives_gpu_layer_t *layer) { return lives_gpu_layer_unpin_impl(layer); }
// the host is about to free or replace this layer's pixel_data itself (weed_layer_pixel_data_free, an error path, a CPU body that
// allocates new planes): drop the device copies WITHOUT bringing them home.  After this no table entry refers to the layer's host
// pointers, so a later allocation at the same address cannot be mistaken for a resident plane.
int lives_gpu_layer_forget(lives_gpu_layer_t *layer) {
  Layer l;
  if (!bound() || !layer) return LGPU_E_BADARG;
  if (read_layer(layer, &l)) for (int p = 0; p < l.nplanes; p++) res_drop(l.pd[p]);
  g_api.leaf_delete(layer, kLeafResident);
  return LGPU_OK;
}
// optional frame allocator pair for lives_gpu_weed_api.pixel_alloc / pixel_free: page-locked, zeroed host memory, so the planes the seam creates
// (and any frame the host allocates through it) cross PCIe by DMA at link rate instead of through the staging chunks.  Freeing a plane through it
// also drops a device copy registered under that address.
static std::mutex g_pinned_mu;
static std::unordered_map<const void *, size_t> g_pinned_blocks;      // blocks handed out by lives_gpu_pinned_calloc: base -> bytes (for the range drop on free)
void *lives_gpu_pinned_calloc(size_t bytes) {
  void *p = lgpu_pinned_calloc(bytes);
  if (p) { std::lock_guard<std::mutex> lk(g_pinned_mu); g_pinned_blocks[p] = bytes ? bytes : 1; }
  return p;
}
void lives_gpu_pinned_free(void *p) {
  size_t bytes = 1;
  if (p) {
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    auto it = g_pinned_blocks.find(p);
    if (it != g_pinned_blocks.end()) { bytes = it->second; g_pinned_blocks.erase(it); }
  }
  if (p) res_drop_range(p, bytes);
  lgpu_pinned_free(p);
}

// residency bridge for the weed plugin (same library, other seam): the device copy of a pinned layer's plane, looked up by the host plane
// pointer the channel carries; NULL when the plane is not resident (or smaller than asked).  Entries exist only between lives_gpu_layer_pin
// and unpin / forget / the release of the plane through this library (free_planes, lives_gpu_pinned_free).
void *lives_gpu_resident_lookup(const void *host_plane, size_t min_bytes) {
  if (!host_plane) return nullptr;
  Dev b;
  if (plane_is_lazy(host_plane) && !lazy_materialise(host_plane)) return nullptr;
  lazy_run_readers_of(host_plane);                    // the caller may write the plane
  const bool found = res_update(host_plane, [&](Dev *e) {
    if (!e || e->bytes < min_bytes) return false;
    b = *e;
    e->stream = nullptr; e->nr = 0;
    return true;
  });
  if (!found) return nullptr;
  // the caller works on the NULL stream: hand the plane over to it (the null stream waits for the plane's writer and readers; the next seam call on a
  // thread's stream will in turn wait for the null stream)
  void *users[5] = {b.stream, b.rs[0], b.rs[1], b.rs[2], b.rs[3]};
  for (int i = 0; i < 1 + b.nr; i++) {
    if (users[i] == nullptr || users[i] == kIdle) continue;
    if (!t_event && lgpu_event_create(&t_event) != LGPU_OK) t_event = nullptr;
    if (!(t_event && lgpu_event_record(t_event, users[i]) == LGPU_OK && lgpu_stream_wait_event(nullptr, t_event) == LGPU_OK)) lgpu_sync(users[i]);
  }
  return b.d;
}
// The same for callers that enqueue on the CALLING THREAD's stream (lives_gpu_thread_stream; what livesgpu_fx.so does): acquire orders that stream behind the
// plane's writer (and, for a write, its readers), release records the use once the caller's work is enqueued.
void *lives_gpu_thread_stream(void) { return ready() ? S() : nullptr; }
void lives_gpu_stream_follow(void *other) { if (ready()) follow(other); }
void *lives_gpu_resident_acquire(const void *host_plane, size_t min_bytes, int write) {
  if (!host_plane || !ready()) return nullptr;
  return acquire(host_plane, min_bytes, write != 0);
}
void lives_gpu_resident_release(const void *host_plane, int write) {
  if (host_plane) touch_done(host_plane, write != 0);
}
void lives_gpu_transfer_stats(unsigned long long *h2d_bytes, unsigned long long *d2h_bytes) {
  if (h2d_bytes) *h2d_bytes = g_h2d.load();
  if (d2h_bytes) *d2h_bytes = g_d2h.load();
}

}  // extern "C"
