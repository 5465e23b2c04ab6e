// seam_resident.h -- the device copies of pinned planes (definitions: seam_resident.cpp): the calling thread's stream and the hand-over between streams, the
// residency table and the ONLY operations that reach one of its entries, the buffer pool, and the per-call unit of device work (struct Work) every seam body
// builds.  Deferred programs (seam_lazy.h) sit in the table as entries of their own; this unit calls into that one through lazy_discard, lazy_run_readers_of and
// lazy_materialise only.
#pragma once
#include <sched.h>
#include <atomic>
#include <mutex>
#include <unordered_map>
#include "seam_weed.h"

#pragma GCC visibility push(hidden)
namespace seam {

// ---- device residency of pinned layers ---------------------------------------------------------------------------------
// A layer the host pinned (lives_gpu_layer_pin) keeps the authoritative copy of its planes in HBM, keyed by the HOST plane
// pointer: uploads of such a plane become device-to-device copies, downloads replace the device copy and leave the host
// bytes stale until lives_gpu_layer_sync().  The CONVERT chain of one plan step (pconv -> gamma -> resize -> letterbox) then
// crosses PCIe once in each direction instead of eight times.

// The calling thread's stream (null until its first use; lifetime and recycling: seam_resident.cpp).  Plain data, so that another unit's S() is a load: the object
// that hands the stream on when the thread ends has a destructor and stays inside seam_resident.cpp
struct ThreadStream { void *stream, *event; bool tried; };
extern __thread ThreadStream t_ts;
void *first_stream();
inline void *S() { return t_ts.tried ? t_ts.stream : first_stream(); }

// A device buffer and the stream its last use was enqueued on.  Ownership of a resident plane moves from call to call; a call on ANOTHER thread's
// stream orders itself behind the previous owner by recording an event on that stream at the moment of the hand-over (everything enqueued there
// so far, which includes the buffer's last use) and waiting for it -- nothing is recorded while a layer stays on one thread (an event per plane and
// call measured 4 - 8 us each on these streams: 9 -> 17 us per seam call).
// `stream` is where the last WRITE (or exclusive use) was enqueued; `rs` are other streams that have enqueued READS since (two effect instances on two pool
// threads may read one layer at the same time): a reader waits for the writer only, a writer for the writer and all readers.
struct Lazy;
// lazy: the plane is not computed yet -- it stands for a pending program (deferred execution, below; d is null then).  external: caller-owned device memory
// (lives_gpu_layer_pin_device) that never enters the pool.  lazy_readers: pending programs of OTHER planes read this one (their layer 2): they run before it is
// written, replaced or dropped.
struct Dev { void *d = nullptr; size_t bytes = 0; void *stream = nullptr; void *rs[4] = {nullptr, nullptr, nullptr, nullptr}; int nr = 0;
             Lazy *lazy = nullptr; bool external = false; int lazy_readers = 0; };
extern char g_idle_tag;
void *const kIdle = &g_idle_tag;                  // Dev::stream of a buffer whose last use is known to be complete (the stream was synchronised since)
// The table lock: a dozen sub-microsecond critical sections per seam call.  A futex mutex here made sixteen host threads run slower than one (every
// contended acquisition a sleep / wake cycle, ~10 us; tools/bench_seam_mt.py: 500 us per call at 16 threads against 10 us alone), so: spin briefly, then yield.
struct SpinLock {
  std::atomic<bool> held{false};
  void lock() {
    for (int spins = 0;; spins++) {
      if (!held.load(std::memory_order_relaxed) && !held.exchange(true, std::memory_order_acquire)) return;
      if (spins < 4000) __builtin_ia32_pause(); else { sched_yield(); spins = 0; }
    }
  }
  void unlock() { held.store(false, std::memory_order_release); }
};
// Resident planes by HOST plane pointer, in 64 SHARDS with a lock each (round 6): sixteen host threads, one per track, each enter the table ~15 times per plan step
// of their track -- behind ONE lock a recorded seam call cost 6-30 us instead of 0.4 (tools/seam_profile.py); the tracks' planes are different allocations and
// land in different shards.  No function holds two shard locks at once.  The buffer pool has a lock of its own.
struct alignas(128) ResShard { SpinLock mu; std::unordered_map<const void *, Dev> m; };
constexpr int kResShards = 64;
extern ResShard g_shards[kResShards];
inline ResShard &shard_of(const void *h) { const uintptr_t a = (uintptr_t)h; return g_shards[((a >> 12) ^ (a >> 18) ^ (a >> 25)) & (kResShards - 1)]; }
extern __thread bool t_pinned;                  // the call in progress works on a pinned layer

// No HIP call is made under a table lock: the functions below copy what they need out of the tables and do the stream work afterwards.
// The calling thread's stream waits for everything enqueued so far on the stream of the buffer's last use, if that is another stream.
void follow_other(void *other);
inline void follow(void *other) {                        // other: a stream (nullptr = the null stream) or kIdle
  if (other == S() || other == kIdle) return;
  follow_other(other);
}
inline void await(const Dev &b, bool write = true) {
  if (!b.d) return;
  follow(b.stream);
  if (write) for (int i = 0; i < b.nr; i++) follow(b.rs[i]);
}
// (the plane's shard lock held) the calling thread's stream has enqueued a read / a write of the buffer
inline void note_use(Dev &e, bool write) {
  void *s = S();
  if (write) { e.stream = s; e.nr = 0; return; }
  if (e.stream == s) return;
  for (int i = 0; i < e.nr; i++) if (e.rs[i] == s) return;
  if (e.nr < 4) e.rs[e.nr++] = s;
  else e.rs[0] = s;                               // a fifth concurrent reader stream of one plane: not tracked (LiVES copies a layer that fans out)
}

// ---- the table's operations: the only ways to an entry.  Each takes ONE shard's lock, once, and makes no HIP call under it; nobody else names a shard. ----
inline bool res_peek(const void *h, Dev *out) {             // copies the entry if there is one
  ResShard &sh = shard_of(h);
  std::lock_guard<SpinLock> lk(sh.mu);
  auto it = sh.m.find(h);
  if (it == sh.m.end()) return false;
  *out = it->second;
  return true;
}
// erases and returns the entry if there is one and take(entry) says so (it may note why not); else an empty Dev.  The callable: as for res_update
template <class F> Dev res_take_if(const void *h, F &&take) {
  Dev b;
  ResShard &sh = shard_of(h);
  std::lock_guard<SpinLock> lk(sh.mu);
  auto it = sh.m.find(h);
  if (it != sh.m.end() && take((const Dev &)it->second)) { b = it->second; sh.m.erase(it); }
  return b;
}
inline Dev res_take(const void *h) { return res_take_if(h, [](const Dev &) { return true; }); }      // erases and returns the entry, or an empty Dev
inline Dev res_swap(const void *h, Dev b) {                 // stores b and returns what was there (an empty Dev: nothing)
  ResShard &sh = shard_of(h);
  std::lock_guard<SpinLock> lk(sh.mu);
  Dev &slot = sh.m[h];
  const Dev old = slot;
  slot = b;
  return old;
}
// f(Dev *) -- nullptr: no entry -- runs under the plane's shard lock; its result is returned.  THE CONTRACT of every callable handed to this header: no HIP call
// (nothing named lgpu_*), no other access to the table, and no allocation that can re-enter the seam (the host's allocator may free planes through it)
template <class F> auto res_update(const void *h, F &&f) -> decltype(f((Dev *)nullptr)) {
  ResShard &sh = shard_of(h);
  std::lock_guard<SpinLock> lk(sh.mu);
  auto it = sh.m.find(h);
  return f(it == sh.m.end() ? (Dev *)nullptr : &it->second);
}
// every entry, shard by shard (one shard's lock at a time): f(host plane, Dev &) answers what happens to the entry, or ends the scan
enum { RES_KEEP = 0, RES_ERASE = 1, RES_STOP = 2 };
template <class F> void res_scan(F &&f) {
  for (ResShard &sh : g_shards) {
    std::lock_guard<SpinLock> lk(sh.mu);
    for (auto it = sh.m.begin(); it != sh.m.end();) {
      const int what = f(it->first, it->second);
      if (what == RES_STOP) return;
      if (what == RES_ERASE) it = sh.m.erase(it); else ++it;
    }
  }
}
inline bool plane_is_lazy(const void *h) { Dev e; return res_peek(h, &e) && e.lazy != nullptr; }

bool pool_take(size_t n, Dev *out);
void pool_give(Dev b);
void res_put(const void *h, Dev b);
void res_drop(const void *h);
void res_drop_range(const void *base, size_t bytes);
void free_planes(const Layer &l);

int lives_gpu_layer_unpin_impl(weed_plant_t *layer);      // lives_gpu_layer_unpin's body (seam_resident.cpp)
struct PinScope {
  bool prev;
  weed_plant_t *layer;
  explicit PinScope(weed_plant_t *layer_) : prev(t_pinned), layer(layer_) { t_pinned = layer && bound() && has_leaf(layer, kLeafResident); }
  ~PinScope() { t_pinned = prev; }
  // every FALSE a seam call returns on a PINNED layer -- declined, or failed after it started (allocation, launch, copy) -- leaves the layer
  // synchronised and unpinned (lives_gpu_layer.h: "the CPU body reads current bytes"); decline() does the same on the paths that know they decline
  int settle(int rc) {
    if (!rc && t_pinned && layer && has_leaf(layer, kLeafResident)) lives_gpu_layer_unpin_impl(layer);
    return rc;
  }
};
// a seam call on `layer`: its body runs with t_pinned set for that layer, and the FALSE it may return is settled
template <class F> int pinned(weed_plant_t *layer, F &&body) {
  PinScope pin(layer);
  return pin.settle(body());
}

inline bool ready() { return bound() && lgpu_init(g_prefs.device) == LGPU_OK; }
inline bool sync() { return lgpu_sync(S()) == LGPU_OK; }

uint8_t *acquire(const void *h, size_t n, bool write);
uint8_t *resident(const void *h, size_t n, bool write);
void touch_done(const void *h, bool write);

// One seam call's device-side work, enqueued on the calling thread's stream.  in(): the current bytes of an existing plane.  out(): a plane
// the call creates (for a new host plane).  inout(): a plane modified in place.  finish() makes the results the planes' contents: downloads + ONE
// sync for an ordinary layer; for a pinned layer the pool buffers the kernels wrote become the resident copies, nothing moves, nothing waits.
// A Work that is dropped without finish() (any failure) gives its buffers back: the layer is as it was.  Either way every resident plane the
// call touched is marked with the calling thread's stream, which is what a later call on another thread's stream orders itself behind.
struct Work {
  struct Out { uint8_t *host; Dev b; size_t n; bool pooled; };
  Out outs[8];
  const void *touched[12];
  bool twrite[12];
  int nout = 0, ntouched = 0;
  bool ok = true, done = false;
  uint8_t *use(const void *h, size_t n, bool write);
  const uint8_t *in(const uint8_t *h, size_t n, int slot);
  uint8_t *out(uint8_t *h, size_t n, int slot, bool zero);
  uint8_t *inout(uint8_t *h, size_t n, int slot);
  void mark_touched();
  bool finish();
  ~Work();
};

lives_gpu_boolean decline(weed_plant_t *layer);

const uint16_t *device_lut16(int from, int to);

}  // namespace seam
#pragma GCC visibility pop
