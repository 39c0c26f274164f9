// kmhg_pool.h -- the device block pool's bookkeeping (host only: no HIP, any C++17 compiler).
//
// Caching allocator: blocks are kept per (device, size class) and reused, so repeated builds and
// queries (bench steps, many queries against one index) pay the device allocation once.
// Stream-ordered releases inside one host call (one build, query, ...) share ONE event: every
// ordered release on the group's stream is deferred to the group's end, where a single event is
// recorded for all of them.  (Each event record is a marker packet the command processor drains
// the stream for; a build used to record ~14 of them back to back.)  A group whose owner has
// already recorded an event of its own behind the group's last work hands that one over
// (ReleaseGroupT::adopt) and the pool records none: the blocks wait for the owner's event, which
// the pool only polls and waits for -- it never records, recycles or keeps it.  The owner keeps
// the event alive, and does not destroy it, for as long as blocks may be pending behind it; it may
// record it again (the entries then wait for that later work too, which is safe).
//
// Same-stream reuse: a pending block remembers the stream its release was ordered behind, and a
// request that names the stream its block is first used on (alloc(bytes, stream)) takes a pending
// block of its class released behind that very stream at once -- no host wait, no event query.
// Stream order already puts every use the new owner queues behind the work the block was released
// behind, so back-to-back builds on one stream reuse each other's blocks while the device is
// still busy with the earlier one, and the host enqueues build i + 1 while build i runs.  Such a
// request polls the pending events only when neither the free list nor that path serves it.  A
// block's first use must then be work queued on that stream: a block first touched by the host
// or by another stream is asked for without one (alloc(bytes)) and waits as before.  A taken
// block that owned its batch's event passes the event on to a block still pending behind it,
// and recycles it only when it was the last (a recycled event may be recorded on another stream,
// so it must not return while a block still waits behind it).  Streams are told apart by their
// handles: a caller that destroys a stream with blocks still pending behind it trims the pool
// first.  How far the host may run ahead of the device is bounded by RecordPool below, not by
// the pool's depth.
//
// The device sits behind `Dev`, a small backend whose stream and event handles are opaque
// pointers (the engine's HipDev; a fake of malloc'ed blocks and scripted events in
// tools/asan/host_check).  A Dev provides
//   int  current()                          the calling thread's device
//   void use(int dev)                       make `dev` current
//   PoolAlloc alloc(size_t sz, void** p, std::string* text)   ok / oom / error with its text
//   void free(void* p)                      a block of the current device
//   void* event()                           a new event, nullptr where none can be made
//   bool record(void* ev, void* stream)     false where it cannot be recorded
//   bool done(void* ev)                     has the work recorded before it completed?
//   void wait_event(void* ev), void wait_stream(void* stream)
//   [[noreturn]] void alloc_failed(PoolAlloc, const std::string& text)    the caller's error
//   static PoolKnobs knobs()                (only for BlockPool::get())
// All control flow is here; nothing here reads the environment.  tools/asan/host_check runs the
// pool under ASan + UBSan against literal scenarios and host_check_tsan runs it from four threads
// (tests/test_pool_host.py, tests/test_pool_stream_reuse.py).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace kmhg {

// The pool's size class of a request.
inline size_t pool_size_class(size_t b) {
  if (b <= (1u << 20)) {           // small: power of two >= 256 B
    size_t r = 256;
    while (r < b) r <<= 1;
    return r;
  }
  const size_t g = 2u << 20;       // large: 2 MiB granules
  return (b + g - 1) / g * g;
}

// The test build's switches of the pool (defaults = the product).
struct PoolKnobs {
  size_t depth = 1;       // KMHG_POOL_DEPTH, 1..8: blocks of a class before a request with no
                          // stream (or another stream's) waits for one; same-stream requests take
                          // a pending block without waiting and never grow past it either
  size_t ahead = 2;       // KMHG_POOL_AHEAD, 1..8: builds freed unwaited that may be unfinished
                          // before the host waits for the oldest (RecordPool)
  bool same_stream = true;   // KMHG_POOL_STREAM=0: off (A/B: every request waits as before)
  bool best_fit = true;   // KMHG_POOL_BESTFIT=0: off
  bool trace = false;     // KMHG_POOL_TRACE: a stderr line per device allocation
};

enum class PoolAlloc { ok, oom, error };

template <class Dev>
struct ReleaseGroupT;

template <class Dev>
class BlockPool {
 public:
  using Key = std::pair<int, size_t>;          // (device, size class)
  struct Block { void* p; Key key; void* ev; bool owns_ev; void* stream = nullptr; };
  struct Snapshot {                            // for tests: every block the pool knows, by state
    std::vector<Block> live, free, pending;
    size_t idle_events, cached;
  };

  explicit BlockPool(PoolKnobs kn = {}, Dev dev = {}) : kn_(kn), dev_(dev) {}
  BlockPool(const BlockPool&) = delete;
  BlockPool& operator=(const BlockPool&) = delete;
  static BlockPool& get() {
    static BlockPool p(Dev::knobs());
    return p;
  }

  // A block first touched by the host or by a stream unknown here: never one that queued work
  // may still use.
  void* alloc(size_t bytes) { return alloc_for(bytes, false, nullptr); }
  // A block whose first use is work queued on `stream` (nullptr: the null stream): it may be one
  // released behind earlier work of that stream, taken without waiting for that work.
  void* alloc(size_t bytes, void* stream) { return alloc_for(bytes, kn_.same_stream, stream); }

 private:
  void* alloc_for(size_t bytes, bool on_stream, void* stream) {
    if (bytes == 0) bytes = 256;
    const Key key{dev_.current(), pool_size_class(bytes)};
    const size_t sz = key.second;
    {
      std::unique_lock<std::mutex> g(mu_);
      if (on_stream) {              // a free block, else the stream's own pending one: no poll
        auto fl = free_.find(key);
        if (fl != free_.end() && !fl->second.empty()) return take(fl);
        if (void* p = take_pending_of(key, stream)) return p;
      }
      poll_pending();
      auto fl = free_.find(key);
      if (fl != free_.end() && !fl->second.empty()) return take(fl);
      // a block of this size still in use by queued work (of another stream, or the request
      // names none): wait for it rather than grow the pool.  Up to depth blocks of a size
      // class exist before a request waits.
      auto n = count_.find(key);
      if (n != count_.end() && n->second >= kn_.depth) {
        for (size_t i = 0; i < pending_.size(); ++i) {
          if (pending_[i].key != key) continue;
          const Block pd = pending_[i];
          pending_.erase(pending_.begin() + (long)i);
          g.unlock();
          dev_.wait_event(pd.ev);
          g.lock();
          if (pd.owns_ev) events_.push_back(pd.ev);
          live_[pd.p] = pd.key;
          return pd.p;
        }
      }
      // a large request with no block of its own size: the smallest idle cached block of at
      // most 1.5x its size serves it (it keeps its own size class and returns to it).  A
      // device allocation of GBs costs ~0.1 ms per GB: the first 500 Mbp query of a process
      // reuses the build's freed 6 GB stream buffers for its records and rows (2 of its 3
      // GB-sized buffers) instead of allocating 10 GB.
      if (kn_.best_fit && sz >= BEST_FIT_MIN) {
        for (auto it = free_.lower_bound(key);
             it != free_.end() && it->first.first == key.first && it->first.second <= sz + sz / 2;
             ++it)
          if (!it->second.empty()) return take(it);
      }
    }
    if (kn_.trace)
      std::fprintf(stderr, "kmhg pool: hipMalloc %zu B on device %d\n", sz, key.first);
    void* p = nullptr;
    std::string text;
    PoolAlloc st = dev_.alloc(sz, &p, &text);
    if (st == PoolAlloc::oom) {   // release the cache and retry once
      trim();
      st = dev_.alloc(sz, &p, &text);
    }
    if (st != PoolAlloc::ok) dev_.alloc_failed(st, text);
    std::lock_guard<std::mutex> g(mu_);
    live_[p] = key;
    ++count_[key];
    return p;
  }

 public:
  // An unordered release returns the block at once.  A stream-ordered one returns it once the
  // work queued on `stream` up to now has completed (an event is recorded and polled on later
  // allocations); inside the thread's open ReleaseGroup of that stream it waits for the group's
  // end.  Unknown and null pointers are ignored.
  void release(void* p, void* stream = nullptr, bool ordered = false) {
    if (!p) return;
    ReleaseGroupT<Dev>* rg = ReleaseGroupT<Dev>::open;
    if (ordered && rg && &rg->pool == this && rg->s == stream) {
      rg->ps.push_back(p);          // deferred to the group's one event
      return;
    }
    if (ordered) release_behind(&p, 1, stream);
    else release_now(&p, 1);
  }
  // blocks still used by work queued on `stream`: one event recorded for all of them.  Where no
  // event can be made or recorded, the stream is waited for instead and they go straight back.
  // With `adopted`, an event the caller owns and has recorded on `stream` behind that work, none
  // is recorded: the blocks wait for the caller's event and no entry owns it.
  void release_behind(void* const* ps, size_t n, void* stream, void* adopted = nullptr) {
    if (n == 0) return;
    if (adopted) {
      std::lock_guard<std::mutex> g(mu_);
      for (size_t i = 0; i < n; ++i) retire(ps[i], adopted, stream);
      return;
    }
    void* ev = recorded_event(stream);
    std::lock_guard<std::mutex> g(mu_);
    const size_t before = pending_.size();
    for (size_t i = 0; i < n; ++i) retire(ps[i], ev, stream);
    if (!ev) return;
    if (pending_.size() > before) pending_.back().owns_ev = true;   // the last one queued
    else events_.push_back(ev);       // nothing queued: the event goes straight back
  }
  // blocks no queued work uses any more (their stream was synchronized)
  void release_now(void* const* ps, size_t n) {
    std::lock_guard<std::mutex> g(mu_);
    for (size_t i = 0; i < n; ++i) retire(ps[i], nullptr);
  }
  // Waits for every pending block and frees all cached ones, each on its own device.  Live
  // blocks are not touched.
  void trim() {
    std::lock_guard<std::mutex> g(mu_);
    for (const Block& pd : pending_) {
      dev_.wait_event(pd.ev);
      settle(pd);
    }
    pending_.clear();
    const int cur = dev_.current();
    for (auto& kv : free_) {
      dev_.use(kv.first.first);
      for (void* p : kv.second) dev_.free(p);
      auto n = count_.find(kv.first);
      if (n != count_.end()) n->second -= std::min(n->second, kv.second.size());
      cached_ -= kv.first.second * kv.second.size();
    }
    free_.clear();
    dev_.use(cur);
  }
  int64_t cached() {
    std::lock_guard<std::mutex> g(mu_);
    return (int64_t)cached_;
  }
  Snapshot snapshot() {
    std::lock_guard<std::mutex> g(mu_);
    Snapshot s{{}, {}, pending_, events_.size(), cached_};
    for (auto& kv : live_) s.live.push_back({kv.first, kv.second, nullptr, false, nullptr});
    for (auto& kv : free_)
      for (void* p : kv.second) s.free.push_back({p, kv.first, nullptr, false, nullptr});
    return s;
  }

 private:
  // Everything below but recorded_event runs with mu_ held.
  using FreeLists = std::map<Key, std::vector<void*>>;
  void* take(typename FreeLists::iterator fl) {     // a cached block (its list not empty) -> live
    void* p = fl->second.back();
    fl->second.pop_back();
    cached_ -= fl->first.second;
    live_[p] = fl->first;
    return p;
  }
  // p leaves live_: behind `ev` into pending_, or with no event straight into its free list
  void retire(void* p, void* ev, void* stream = nullptr) {
    auto it = live_.find(p);
    if (it == live_.end()) return;
    const Block b{p, it->second, ev, false, stream};
    live_.erase(it);
    if (ev) pending_.push_back(b);
    else settle(b);
  }
  // a block whose event (if any) has completed returns to its free list; the entry of a batch
  // that owns the shared event recycles it (no create / destroy per release).  An entry polled
  // after its batch's event was recycled and recorded again only waits for later work (safe).
  void settle(const Block& b) {
    if (b.owns_ev) events_.push_back(b.ev);
    free_[b.key].push_back(b.p);
    cached_ += b.key.second;
  }
  // The oldest pending block of (device, class) `key` released behind `stream`, taken while the
  // work it waits for may still run: the caller's first use is queued on that stream, behind it.
  // No wait and no query.  The batch's event, where this block owned it, goes to a block still
  // pending behind it; the last one recycles it.
  void* take_pending_of(const Key& key, void* stream) {
    for (size_t i = 0; i < pending_.size(); ++i) {
      if (pending_[i].key != key || pending_[i].stream != stream) continue;
      const Block pd = pending_[i];
      pending_.erase(pending_.begin() + (long)i);
      if (pd.owns_ev) {
        size_t heir = pending_.size();
        for (size_t j = 0; j < pending_.size() && heir == pending_.size(); ++j)
          if (pending_[j].ev == pd.ev) heir = j;
        if (heir < pending_.size()) pending_[heir].owns_ev = true;
        else events_.push_back(pd.ev);
      }
      live_[pd.p] = pd.key;
      return pd.p;
    }
    return nullptr;
  }
  // Each distinct event is queried once per poll (the blocks of one build share one).
  void poll_pending() {
    std::vector<std::pair<void*, bool>> seen;
    const auto done = [&](void* ev) {
      for (const auto& e : seen)
        if (e.first == ev) return e.second;
      seen.emplace_back(ev, dev_.done(ev));
      return seen.back().second;
    };
    for (size_t i = 0; i < pending_.size();) {
      if (done(pending_[i].ev)) {
        settle(pending_[i]);
        pending_[i] = pending_.back();
        pending_.pop_back();
      } else {
        ++i;
      }
    }
  }
  // An event (recycled if one is idle) recorded on `stream`; where none can be made or recorded,
  // the stream is waited for instead and nullptr returned.  Takes mu_ itself: call unlocked.
  void* recorded_event(void* stream) {
    void* ev = nullptr;
    {
      std::lock_guard<std::mutex> g(mu_);
      if (!events_.empty()) { ev = events_.back(); events_.pop_back(); }
    }
    if (!ev) ev = dev_.event();
    if (!ev || !dev_.record(ev, stream)) {
      dev_.wait_stream(stream);
      if (ev) { std::lock_guard<std::mutex> g(mu_); events_.push_back(ev); }
      ev = nullptr;
    }
    return ev;
  }

  static constexpr size_t BEST_FIT_MIN = (size_t)256 << 20;
  const PoolKnobs kn_;
  Dev dev_;
  std::mutex mu_;
  FreeLists free_;
  std::map<Key, size_t> count_;      // blocks of each size class (any state)
  std::map<void*, Key> live_;
  std::vector<Block> pending_;
  std::vector<void*> events_;        // idle events
  size_t cached_ = 0;                // bytes in free_
};

// The ordered releases of one host call on its stream, collected on the calling thread and
// returned to the pool together at the scope's end (groups nest; the innermost is the open one).
template <class Dev>
struct ReleaseGroupT {
  static inline thread_local ReleaseGroupT* open = nullptr;
  BlockPool<Dev>& pool;
  void* s;
  std::vector<void*> ps;
  ReleaseGroupT* prev;
  // set after a synchronize of `s` with no launch behind it: the blocks go straight back to the
  // pool, no event (a synchronous call's last step)
  bool synced = false;
  // the owner's event, recorded on `s` behind the last work that uses the group's blocks (adopt)
  void* adopted = nullptr;
  ReleaseGroupT(BlockPool<Dev>& pl, void* stream) : pool(pl), s(stream), prev(open) { open = this; }
  explicit ReleaseGroupT(void* stream) : ReleaseGroupT(BlockPool<Dev>::get(), stream) {}
  ~ReleaseGroupT() {
    open = prev;
    if (synced) pool.release_now(ps.data(), ps.size());
    else pool.release_behind(ps.data(), ps.size(), s, adopted);
  }
  // The group's blocks wait for `ev` instead of an event of the pool's: the caller has recorded it
  // on `s`, launches nothing more that uses the blocks before the group ends, and keeps it alive.
  void adopt(void* ev) { adopted = ev; }
  ReleaseGroupT(const ReleaseGroupT&) = delete;
  ReleaseGroupT& operator=(const ReleaseGroupT&) = delete;
};

// Records that carry an event each (`Rec::ev`; the engine's pinned build records), and the bound
// on how far the host runs ahead of the device: a record given back in flight (its build freed
// before anyone waited for it) is pending until its event has completed, and while `ahead` of
// them are pending a take waits for the oldest one's event first.  With same-stream block reuse
// no allocation waits between such builds any more; this wait is the back-pressure.  Pending
// records are kept oldest first.  `grow(std::vector<Rec>&)` makes more records when none is free.
template <class Dev, class Rec>
class RecordPool {
 public:
  explicit RecordPool(size_t ahead = PoolKnobs{}.ahead, Dev dev = {})
      : ahead_(std::max<size_t>(ahead, 1)), dev_(dev) {}
  RecordPool(const RecordPool&) = delete;
  RecordPool& operator=(const RecordPool&) = delete;
  template <class Grow>
  Rec take(Grow&& grow) {
    std::unique_lock<std::mutex> g(mu_);
    for (size_t i = 0; i < pending_.size();) {
      if (dev_.done(pending_[i].ev)) {
        free_.push_back(pending_[i]);
        pending_.erase(pending_.begin() + (long)i);
      } else {
        ++i;
      }
    }
    while (pending_.size() >= ahead_) {
      const Rec r = pending_.front();
      pending_.erase(pending_.begin());
      g.unlock();
      dev_.wait_event(r.ev);
      g.lock();
      free_.push_back(r);
    }
    if (free_.empty()) grow(free_);
    const Rec r = free_.back();
    free_.pop_back();
    return r;
  }
  void give(const Rec& r, bool in_flight) {
    std::lock_guard<std::mutex> g(mu_);
    (in_flight ? pending_ : free_).push_back(r);
  }
  std::pair<size_t, size_t> sizes() {       // for tests: free, pending
    std::lock_guard<std::mutex> g(mu_);
    return {free_.size(), pending_.size()};
  }

 private:
  const size_t ahead_;
  Dev dev_;
  std::mutex mu_;
  std::vector<Rec> free_, pending_;
};

}  // namespace kmhg
