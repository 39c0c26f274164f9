// kmhg_engine.cpp -- host orchestrator of the MI355X k-mer position index + the C-ABI.
//
// Runtime pieces (native, as the reference's C core is native):
//   * DevicePool   caching device allocator: BlockPool (kmhg_pool.h, all of its bookkeeping)
//                  over the HipDev backend below
//   * Timing       per-kernel HIP-event pairs on the launch stream (kmhg_timing_*)
//   * Index/Query  build -> query -> readout pipelines over kmhg_kernels.hip
// Reference entry points each C function replaces are listed in include/kmhgpu.h.
#include <atomic>
#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "kmhg_common.h"
#include "kmhg_blocks.h"
#include "kmhg_chains.h"
#include "kmhg_kernels.h"
#include "kmhg_plan.h"
#include "kmhg_hostwork.h"
#include "kmhg_pool.h"
#include "kmhg_reads.h"
#include "kmhg_querycall.h"
#include "kmhg_readsq.h"
#include "kmhg_readsq_dev.h"
#include "kmhg_minimizer.h"
#include "kmhg_segrec.h"
#include "kmhg_parts_read.h"
#include "kmhg_fastx.h"
#include "kmhg_khash.h"
#include "kmhg_sh.h"

// Environment knobs.  The product library reads four: KMHG_TIMING (per-kernel events),
// KMHG_DEVICES (multi-device query), KMHG_ROW_ORDER and KMHG_D2H_THREADS.  Everything else exists
// only in the test build (-DKMHG_TEST_BUILD: libkmhgpu_test.so, which the GPU suite loads for the
// tests that force a path, tests/conftest.py `test_lib`): the path selectors that force each
// build / query / counts path against the oracle (the partitioned build's: BuildKnobs,
// kmhg_plan.h, filled by read_build_knobs below; KMHG_BUILD, KMHG_TEST_BALLOT, KMHG_QUERY_TAGS,
// KMHG_QUERY_DIAG, KMHG_DIAG_CODES, KMHG_COUNT_TABLE, KMHG_COUNT_WALK, KMHG_CO_GLOBAL,
// KMHG_ROW_ORDER_SORT, KMHG_SLICE_POISON, KMHG_TEST_REPLICA), which choose
// between equivalent paths and change no result; fault injection (KMHG_TEST_DISORDER); and the
// A/B-only switches (KMHG_D2H, KMHG_D2H_HUGE, KMHG_HOST_RUNS, KMHG_HOST_PAIRS, KMHG_HOST_POOL,
// KMHG_COUNT_BID, KMHG_RK_CAP, KMHG_SH_SPAN (the span_max given to read_batches, kmhg_reads.h),
// KMHG_POOL_DEPTH, KMHG_POOL_AHEAD, KMHG_POOL_STREAM, KMHG_POOL_BESTFIT, KMHG_POOL_TRACE (the
// pool's: PoolKnobs, kmhg_pool.h, filled once by HipDev::knobs below)).
namespace kmhg {
inline const char* test_build_knob(const char* name) {
#ifdef KMHG_TEST_BUILD
  return std::getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}
}  // namespace kmhg
#include "../../include/kmhgpu.h"

using namespace kmhg;

// ============================================================================ errors
static thread_local std::string g_err;

namespace {

struct Error {
  int code;
  std::string msg;
};

[[noreturn]] void fail(int code, const std::string& msg) { throw Error{code, msg}; }

void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) {
    if (e == hipErrorOutOfMemory) fail(KMHG_ENOMEM, std::string(what) + ": out of device memory");
    fail(KMHG_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
  }
}
#define HIPC(x) hip_check((x), #x)

template <class F>
int guarded(F&& f) {
  try {
    f();
    return KMHG_OK;
  } catch (const Error& e) {
    g_err = e.msg;
    return e.code;
  } catch (const std::bad_alloc&) {
    g_err = "host allocation failed";
    return KMHG_ENOMEM;
  }
}

// ============================================================================ device pool
// BlockPool (kmhg_pool.h) over HIP.  Events carry no timing and no system-scope fence; an
// out-of-memory answer is cleared from the runtime's last-error slot, since the pool trims its
// cache and asks again.
struct HipDev {
  static PoolKnobs knobs() {   // test build: KMHG_POOL_DEPTH / _AHEAD / _STREAM / _BESTFIT / _TRACE
    PoolKnobs kn;
    if (const char* e = test_build_knob("KMHG_POOL_DEPTH"))
      kn.depth = (size_t)std::max(1, std::min(8, std::atoi(e)));
    if (const char* e = test_build_knob("KMHG_POOL_AHEAD"))
      kn.ahead = (size_t)std::max(1, std::min(8, std::atoi(e)));
    if (const char* e = test_build_knob("KMHG_POOL_STREAM")) kn.same_stream = e[0] != '0';
    if (const char* e = test_build_knob("KMHG_POOL_BESTFIT")) kn.best_fit = e[0] != '0';
    kn.trace = test_build_knob("KMHG_POOL_TRACE") != nullptr;
    return kn;
  }
  int current() { int dev = 0; HIPC(hipGetDevice(&dev)); return dev; }
  void use(int dev) { (void)hipSetDevice(dev); }
  PoolAlloc alloc(size_t sz, void** p, std::string* text) {
    const hipError_t e = hipMalloc(p, sz);
    if (e == hipSuccess) return PoolAlloc::ok;
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return PoolAlloc::oom; }
    *text = hipGetErrorString(e);
    return PoolAlloc::error;
  }
  void free(void* p) { (void)hipFree(p); }
  // No system-scope fence at the record (like the timing events below): a release event only
  // gates the reuse of device blocks, by later device work and by the pool's hipEventQuery /
  // hipEventSynchronize on the host.  Nothing is read through it, so no cache has to be written
  // back or invalidated for it.  A runtime that refuses the flag gets the plain event.
  void* event() {
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming | hipEventDisableSystemFence) ==
        hipSuccess)
      return ev;
    (void)hipGetLastError();
    return hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess ? ev : nullptr;
  }
  bool record(void* ev, void* s) {
    return hipEventRecord(static_cast<hipEvent_t>(ev), static_cast<hipStream_t>(s)) == hipSuccess;
  }
  bool done(void* ev) { return hipEventQuery(static_cast<hipEvent_t>(ev)) == hipSuccess; }
  void wait_event(void* ev) { (void)hipEventSynchronize(static_cast<hipEvent_t>(ev)); }
  void wait_stream(void* s) { (void)hipStreamSynchronize(static_cast<hipStream_t>(s)); }
  [[noreturn]] void alloc_failed(PoolAlloc st, const std::string& text) {
    if (st == PoolAlloc::oom) fail(KMHG_ENOMEM, "hipMalloc: out of device memory");
    fail(KMHG_EDEVICE, "hipMalloc: " + text);
  }
};
using DevicePool = BlockPool<HipDev>;
using ReleaseGroup = ReleaseGroupT<HipDev>;

// The stream a new buffer is first used on: every first touch of it is a kernel, memset or copy
// queued on `s`.  The pool may then hand out a block that earlier work of `s` still uses, with
// no host wait (kmhg_pool.h, same-stream reuse).  A buffer first touched by the host, by a copy
// with no stream or by another stream is made without it.
struct FirstUseOn {
  hipStream_t s;
};

// RAII device buffer from the pool.  A buffer bound to a stream is released stream-ordered
// (kernels still queued on that stream may use it after the C++ object dies).
template <class T>
struct DBuf {
  T* p = nullptr;
  size_t n = 0;
  hipStream_t s = nullptr;
  bool ordered = false;
  DBuf() = default;
  explicit DBuf(size_t count) { reset(count); }
  DBuf(size_t count, hipStream_t stream) { reset(count); bind(stream); }
  DBuf(size_t count, FirstUseOn on) { reset(count, on); }
  ~DBuf() { free(); }
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  void bind(hipStream_t stream) { s = stream; ordered = true; }
  void reset(size_t count) {
    free();
    n = count;
    p = static_cast<T*>(DevicePool::get().alloc(std::max<size_t>(count, 1) * sizeof(T)));
  }
  // first used on on.s, and bound to it: released stream-ordered from here on
  void reset(size_t count, FirstUseOn on) {
    free();
    n = count;
    p = static_cast<T*>(DevicePool::get().alloc(std::max<size_t>(count, 1) * sizeof(T), on.s));
    bind(on.s);
  }
  void free() {
    if (p) DevicePool::get().release(p, s, ordered);
    p = nullptr; n = 0;
  }
  size_t bytes() const { return n * sizeof(T); }
  void swap_with(DBuf& o) {
    std::swap(p, o.p);
    std::swap(n, o.n);
    std::swap(s, o.s);
    std::swap(ordered, o.ordered);
  }
};

// Pinned, device-visible host records for the build totals: V_stats writes one directly, so the
// host reads U / N / P with no copy launch.  Each record carries an event recorded after the
// build's last kernel; a record given back while its build is still in flight (an index freed
// before it was ever used) is reused only once that event has completed.
struct PinnedRec {
  BuildMeta* meta = nullptr;
  hipEvent_t ev = nullptr;
};
class PinnedPool {
 public:
  static PinnedPool& get() {
    static PinnedPool p;
    return p;
  }
  // At most PoolKnobs::ahead builds freed unwaited are unfinished when this returns (RecordPool,
  // kmhg_pool.h): a further take waits for the oldest one's event.
  PinnedRec take() {
    PinnedRec r = recs_.take([](std::vector<PinnedRec>& out) {
      constexpr int kSlots = 64;
      BuildMeta* blk = nullptr;
      HIPC(hipHostMalloc(reinterpret_cast<void**>(&blk), sizeof(BuildMeta) * kSlots,
                         hipHostMallocCoherent));
      for (int i = 0; i < kSlots; ++i) {
        PinnedRec r;
        r.meta = blk + i;
        // with its system-scope fence, unlike the pool's release events: the host reads the
        // record behind this event.  (Without it the 10 Mbp build measured 0.1744 against 0.1771
        // ms, the two sets of runs overlapping: not kept)
        HIPC(hipEventCreateWithFlags(&r.ev, hipEventDisableTiming));
        out.push_back(r);
      }
    });
    std::memset(r.meta, 0, sizeof(*r.meta));
    return r;
  }
  void give(PinnedRec r, bool in_flight) {
    if (!r.meta) return;
    recs_.give(r, in_flight);
  }

 private:
  RecordPool<HipDev, PinnedRec> recs_{HipDev::knobs().ahead};
};
// returns a record taken for a host round trip that the scope waited for (any exit path)
// On an exception path the device may still write into the record (a queued scan's total), so
// the stream is drained first: a record back in the free list is never a DMA target.
struct GiveBack {
  PinnedRec& r;
  hipStream_t s;
  ~GiveBack() {
    if (std::uncaught_exceptions() > 0) (void)hipStreamSynchronize(s);
    PinnedPool::get().give(r, false);
  }
};

// ============================================================================ timing
struct Timing {
  static Timing& get() {
    static Timing t;
    return t;
  }
  bool on = false;
  std::string only;                   // record just this kernel (empty = every kernel)
  struct Rec { std::string name; hipEvent_t a, b; };
  std::vector<Rec> recs;
  std::map<std::string, std::pair<int64_t, double>> acc;
  std::mutex mu;

  Timing() {
    const char* e = std::getenv("KMHG_TIMING");
    on = e && e[0] == '1';
  }
  std::vector<hipEvent_t> pool;       // recycled events: no create/destroy per launch
  hipEvent_t take() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e;
    // timing-only events: no system-scope fence (a default event writes back / invalidates the
    // caches at every record, ~10 us of dead time between the kernels it brackets)
    if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) {
      (void)hipGetLastError();
      HIPC(hipEventCreate(&e));
    }
    return e;
  }
  template <class F>
  void run(const char* name, hipStream_t s, F&& launch) {
    if (!on || (!only.empty() && only != name)) { launch(); HIPC(hipGetLastError()); return; }
    hipEvent_t a, b;
    {
      std::lock_guard<std::mutex> g(mu);
      a = take();
      b = take();
    }
    HIPC(hipEventRecord(a, s));
    launch();
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(b, s));
    std::lock_guard<std::mutex> g(mu);
    recs.push_back({name, a, b});
  }
  void collect() {   // resolve recorded events (synchronises on them)
    std::lock_guard<std::mutex> g(mu);
    for (auto& r : recs) {
      (void)hipEventSynchronize(r.b);
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, r.a, r.b);
      auto& x = acc[r.name];
      x.first += 1;
      x.second += ms;
      pool.push_back(r.a);
      pool.push_back(r.b);
    }
    recs.clear();
  }
};
#define LAUNCH(name, stream, ...) Timing::get().run(name, stream, [&] { __VA_ARGS__; })

// One library stream per device for host-pointer entry points.
hipStream_t lib_stream() {
  static std::mutex mu;
  static std::map<int, hipStream_t> streams;
  int dev = 0;
  HIPC(hipGetDevice(&dev));
  std::lock_guard<std::mutex> g(mu);
  auto it = streams.find(dev);
  if (it != streams.end()) return it->second;
  hipStream_t s;
  HIPC(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  streams[dev] = s;
  return s;
}

// KMHG_HOST_POOL=0 (test build): HostPool (kmhg_hostwork.h) starts a thread per task for every
// job, not only for the GB-scale ones (A/B)
static bool fresh_threads() {
  const char* pe = test_build_knob("KMHG_HOST_POOL");
  return pe && pe[0] == '0';
}

// Device -> pageable host copy for the host-pointer entry points (R matrices, numpy arrays):
// results above D2H_STAGE_MIN go through two pinned chunks, the DMA of chunk i + 1 overlapping
// the host copy of chunk i, which d2h_threads() threads split (they also take the destination's
// first-touch page faults in parallel).  Synchronous: returns once dst holds the bytes.
constexpr size_t D2H_CHUNK = 16u << 20;
constexpr size_t D2H_STAGE_MIN = 4u << 20;
// KMHG_D2H_THREADS (A/B), default 8: A/B in one run (`profiles/rd4n_ab_d2h.log`, config 2
// host-boundary query, 10 M rows into a fresh array): 4 threads 7.9 / 8.4 ms, 8 threads 7.0 /
// 6.7 ms, 16 threads 7.7 / 10.1 ms
static int d2h_threads() {
  static const int n = [] {
    const char* e = std::getenv("KMHG_D2H_THREADS");
    return e ? std::max(1, std::min(16, std::atoi(e))) : 8;
  }();
  return n;
}

static void host_copy_par(char* dst, const char* src, size_t n) {
  for_stripes(n, d2h_threads(), 4096, fresh_threads(),
              [=](uint64_t a, uint64_t b) { std::memcpy(dst + a, src + a, b - a); });
}

struct PinStage {
  std::mutex mu;
  char* pin[2] = {nullptr, nullptr};
};
static PinStage& pin_stage() {           // the device's two pinned D2H_CHUNK buffers
  static std::mutex map_mu;
  static std::map<int, PinStage> stages;
  int dev = 0;
  HIPC(hipGetDevice(&dev));
  std::lock_guard<std::mutex> g(map_mu);
  return stages[dev];
}

// A result matrix is usually fresh memory of the caller's allocator (R's allocMatrix: malloc,
// 4-KB pages), so the copy below takes one page fault per 4 KB.  Asking for transparent huge
// pages on the destination's whole 2-MB spans first (madvise(MADV_HUGEPAGE): a hint on the
// mapping, no change to its contents or ownership) makes that one fault per 2 MB.  Measured on
// the box (tools/host_thp_probe.py, profiles/r6r_thp.json, 10 M rows = 80 MB into a fresh
// array): 7.49 ms with 4-KB pages, 2.82 ms with huge pages (numpy asks for them itself).
// KMHG_D2H_HUGE=0 (test build) leaves the destination alone (A/B).
static void hint_huge_pages(void* dst, size_t bytes) {
  static const bool on = [] {
    const char* e = test_build_knob("KMHG_D2H_HUGE");
    return !(e && e[0] == '0');
  }();
  const Span h = on ? huge_span(dst, bytes) : Span{0, 0};
  if (h.len) (void)madvise(reinterpret_cast<void*>(h.begin), h.len, MADV_HUGEPAGE);   // a hint only
}

void d2h_host(void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (!bytes) return;
  static const bool staged = [] {
    const char* e = test_build_knob("KMHG_D2H");      // A/B knob: "direct" = one hipMemcpy
    return !(e && std::string(e) == "direct");
  }();
  hint_huge_pages(dst, bytes);
  if (!staged || bytes < D2H_STAGE_MIN) {
    HIPC(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    return;
  }
  // two pinned chunks per device, so the parts of a multi-device query copy out concurrently
  PinStage& st = pin_stage();
  std::lock_guard<std::mutex> g(st.mu);
  char** pin = st.pin;
  if (!pin[0])
    for (int i = 0; i < 2; ++i)
      HIPC(hipHostMalloc(reinterpret_cast<void**>(&pin[i]), D2H_CHUNK, hipHostMallocPortable));
  // the two events, destroyed on every exit; on an exception the stream is drained first so no
  // DMA into the static pinned chunks is still in flight when the next caller takes them
  struct Ev2 {
    hipEvent_t e[2] = {nullptr, nullptr};
    hipStream_t s;
    ~Ev2() {
      if (std::uncaught_exceptions() > 0) (void)hipStreamSynchronize(s);
      for (auto x : e)
        if (x) (void)hipEventDestroy(x);
    }
  } evs{{nullptr, nullptr}, s};
  hipEvent_t* ev = evs.e;
  for (int i = 0; i < 2; ++i) HIPC(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
  const size_t nch = (bytes + D2H_CHUNK - 1) / D2H_CHUNK;
  auto issue = [&](size_t i) {
    const size_t off = i * D2H_CHUNK, n = std::min(D2H_CHUNK, bytes - off);
    HIPC(hipMemcpyAsync(pin[i & 1], static_cast<const char*>(src) + off, n,
                        hipMemcpyDeviceToHost, s));
    HIPC(hipEventRecord(ev[i & 1], s));
  };
  issue(0);
  if (nch > 1) issue(1);
  for (size_t i = 0; i < nch; ++i) {
    HIPC(hipEventSynchronize(ev[i & 1]));
    const size_t off = i * D2H_CHUNK, n = std::min(D2H_CHUNK, bytes - off);
    host_copy_par(static_cast<char*>(dst) + off, pin[i & 1], n);
    if (i + 2 < nch) issue(i + 2);
  }
}

struct PinRuns {
  std::mutex mu;
  int32_t* p = nullptr;
  size_t cap = 0;                                       // int32 words
};
static PinRuns& pin_runs() {                            // the device's pinned run buffer
  static std::mutex map_mu;
  static std::map<int, PinRuns> bufs;
  int dev = 0;
  HIPC(hipGetDevice(&dev));
  std::lock_guard<std::mutex> g(map_mu);
  return bufs[dev];
}

// The runs of H rows: their count per tile, scanned in place (what k_runs_emit reads), and their
// number, which the scan writes to the pinned `total`.  tiles: H / TILE rounded up + the scan's
// scratch.  Waits for the stream.
uint64_t count_runs(const int2* d_rows, uint64_t H, uint64_t* tiles, uint64_t* total,
                    hipStream_t s) {
  const uint64_t nt = (H + TILE - 1) / TILE;
  LAUNCH("k_runs_count", s, launch_runs_count(d_rows, H, tiles, s));
  LAUNCH("k_scan_tiles_u64", s, launch_scan_u64(tiles, nt, total, tiles + nt, s));
  HIPC(hipStreamSynchronize(s));
  return __atomic_load_n(total, __ATOMIC_ACQUIRE);
}

// Query rows into a host matrix (kmhg_query_fill, the R matrix of seq.kmer.pos): from
// RUNS_HOST_MIN rows on as runs that host threads expand (kmhg_hostwork.h), unless the rows do
// not shrink RUNS_HOST_GAIN-fold; else d2h_host.  KMHG_HOST_RUNS=0 (test build): always d2h_host
// (A/B).
void rows_to_host(const int2* d_rows, uint64_t H, int32_t* dst, hipStream_t s) {
  if (!H) return;
  const char* hre = test_build_knob("KMHG_HOST_RUNS");    // (read per call: tests flip it)
  const bool runs_on = !(hre && hre[0] == '0');
  if (!runs_on || H < RUNS_HOST_MIN || H > INT32_MAX) {
    d2h_host(dst, d_rows, H * 8, s);
    return;
  }
  ReleaseGroup rg(s);
  const uint64_t nt = (H + TILE - 1) / TILE;
  DBuf<uint64_t> tiles(nt + scan_u64_scratch(nt), s);
  PinnedRec hrec = PinnedPool::get().take();
  GiveBack give_back{hrec, s};
  const uint64_t n = count_runs(d_rows, H, tiles.p, &hrec.meta->n_kmers, s);
  if (n * 12 * RUNS_HOST_GAIN > H * 8) {                // runs would not pay: the rows
    d2h_host(dst, d_rows, H * 8, s);
    return;
  }
  DBuf<int32_t> druns(3 * n, s);
  LAUNCH("k_runs_emit", s, launch_runs_emit(d_rows, H, tiles.p, druns.p, s));
  PinRuns& pr = pin_runs();
  std::lock_guard<std::mutex> g(pr.mu);
  if (pr.cap < 3 * n) {
    if (pr.p) HIPC(hipHostFree(pr.p));                  // (no copy into it is in flight)
    pr.p = nullptr;
    pr.cap = 0;
    const size_t cap = std::max<size_t>(3 * n, 3u << 20);
    HIPC(hipHostMalloc(reinterpret_cast<void**>(&pr.p), cap * 4, hipHostMallocPortable));
    pr.cap = cap;
  }
  HIPC(hipMemcpyAsync(pr.p, druns.p, 3 * n * 4, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  hint_huge_pages(dst, H * 8);
  expand_runs_host(pr.p, n, H, dst, expand_threads(H * 8), fresh_threads());
}

// Pageable host -> device copy for the host-pointer entry points (the R string of make.kmer.hash
// / seq.kmer.pos), ordered on `s`.
void h2d_host(void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (!bytes) return;
  // pageable: the runtime stages it at the link's rate (10 MB in 0.194 ms, 54 GB/s,
  // tools/h2d_probe.hip).  Measured and removed: two pinned chunks filled by host threads while
  // the previous chunk's DMA runs (round 3: 0.81-0.92 ms against 0.63 for the config-2 host
  // build), and pinning the caller's pages in place (hipHostRegister: the same 0.194 ms).
  HIPC(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
}

// KMHG_ROW_ORDER=khash makes new indices label kmer.pos rows in the reference's khash order.
int default_row_order() {
  const char* e = std::getenv("KMHG_ROW_ORDER");
  return (e && std::string(e) == "khash") ? KMHG_ORDER_KHASH : KMHG_ORDER_FIRST;
}

struct Canon {              // readout order arrays (first occurrence or khash), built on use
  bool ready = false;
  int order = KMHG_ORDER_FIRST;   // which order the arrays below hold
  DBuf<uint32_t> perm, canon_off, pkeys;
  DBuf<uint64_t> pair_off;
  DBuf<uint2> rinfo;        // {count, aux} of each row's slot (readout kernels read rows in order)
  uint64_t n_multi = 0;
};

}  // namespace

// ============================================================================ objects
struct kmhg_index {
  int k = 0;
  int device = 0;
  hipStream_t stream = nullptr;   // last stream the index was used on (ordered release)
  int64_t L = 0;
  Geom geom{1, 1};             // nb buckets x capb slots (+1 side slot)
  uint64_t U = 0, N = 0, P = 0;
  uint64_t slots() const { return (uint64_t)geom.nb * geom.capb + 1; }
  uint32_t max_n = 0;
  DBuf<Slot> table;
  DBuf<int32_t> positions;
  Canon canon;
  int row_order = default_row_order();   // kmer.pos k-mer order (KMHG_ORDER_*)
  // kmhg_set_max_occ: the query entries' occurrence cap, 0 = none.  An entry reads it once
  // (capped); a replica's own copy is never looked at -- its calls carry the home index's.
  std::atomic<int64_t> max_occ{0};
  // kmhg_build_sampled*: the (w,k)-minimizer sampling the index was built with (kmhg_minimizer.h);
  // 1: every valid window.  A query at the index's own k applies the same rule to its sequence.
  int sampling = 1;
  // asynchronous build (kmhg_build_device returns before the kernels finish): the totals land
  // in `rec`; `src` is kept for the overflow fallback until finish_build()
  bool pending = false;
  PinnedRec rec;
  const uint8_t* src = nullptr;
  // counts index (count.kmers, kmhg_count.hip): sources > 0.  `positions` then holds the
  // U x sources count matrix (row-major, rows_cap allocated), `ckeys` the keys of the rows,
  // slot_row / row_slot the table <-> row maps.  count.kmers rows are appended in slot order with
  // their insertion-order keys `rord`; before a readout, `rorder` (first-insertion rank -> row)
  // is derived from them (ensure_row_order; order_ready) -- the rows themselves never move.  A
  // suffix hash's rows are order-free (no rord, no rorder).
  uint32_t sources = 0;
  bool canonical = false;         // suffix hash (count.kmers.fq.sh.rp): canonical k-mer counts
  bool single = false;            // ... the single suffix_hash of count.kmers.fq.sh (kind 3)
  uint64_t rows_cap = 0, kmer_count = 0;
  bool u_upper = false;           // U is only an upper bound (batch table of the global fallback)
  // last read batch (kmhg_sh_last_batch): HLL distinct estimate, bucket spread, build path
  double co_est = 0;
  int co_spread = 0, co_path = 0;
  DBuf<uint64_t> ckeys, rord;
  DBuf<uint32_t> rorder;
  bool order_ready = true;
  // per-bucket statistics of a partitioned build (bstats_nb buckets, 0 for other builds): a
  // batch index adopted by a counts index takes its row offsets from them (k_count_walk_b)
  DBuf<BucketStats> bstats;
  uint32_t bstats_nb = 0;
  DBuf<uint32_t> slot_row, row_slot;
  // seq.kmer.pos diagonal path (DiagIdx, kmhg_kernels.h): the index sequence's 2-bit code words
  // and window bits, written by the build (V_hist0); the bits of repeated keys' windows are
  // cleared and the slot tags built on the first eligible query (V_diag_prep)
  DBuf<uint64_t> dcodes;
  DBuf<uint8_t> ptag;             // one tag byte per table slot (0 = empty)
  // part of an owner-computes build (kmhg_build_device_part): holds buckets
  // [geom.b0, geom.b0 + geom.nb) of a table of geom.nbh buckets; exported for an assembly, or
  // queried in place by the owner-routed query (kmhg_query_run_device_part)
  bool is_part = false;
  // ps_ready: published (release) after the preparing query's synchronize; read (acquire) by
  // later queries, possibly on other threads, before they use ptag / the uniq bits
  std::atomic<bool> ps_ready{false};
  // how the index was built (kmhg_info.build / .fallback): KMHG_BUILD_* and whether
  // finish_build() had to rebuild it with the global-atomic build
  int build_kind = 0;
  int fallback = 0;
  // copies of this index on other devices for multi-device queries (KMHG_DEVICES), keyed by
  // device (one per device); made on first use by peer copies over xGMI, freed with the index
  std::map<int, kmhg_index*> replicas;
  std::mutex rep_mu;
  bool ps_failed = false;                 // guarded by ps_mu
  // the build wrote ptag and the repeated keys' window bits (build_device_v2, build-time tags):
  // the first diagonal query derives uniq alone (V_diag_valid)
  bool tags_built = false;
  std::mutex ps_mu;
  DiagBlock diag_block_of() const { return diag_block(dcodes.p, L - k + 1); }
  DiagIdx diag_view() const {
    const DiagBlock b = diag_block_of();
    return DiagIdx{b.code, b.uniq, L - k + 1};
  }
  // stream-ordered release of everything the index holds (work queued on `s` may still read it)
  void bind_all(hipStream_t s) {
    table.bind(s); positions.bind(s); ckeys.bind(s); rord.bind(s); rorder.bind(s); bstats.bind(s);
    slot_row.bind(s);
    row_slot.bind(s); dcodes.bind(s); ptag.bind(s);
    canon.perm.bind(s); canon.canon_off.bind(s); canon.pkeys.bind(s); canon.pair_off.bind(s);
    canon.rinfo.bind(s);
  }
};

struct kmhg_query {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t H = 0;
  DBuf<int2> rows;
  // multi-device query (KMHG_DEVICES): one part per device, each holding the rows of its
  // contiguous window range in its own HBM; part i's rows start at row part_off[i].  `rows`
  // then stays empty until a device-side reader asks for them on `device` (gathered once).
  std::vector<kmhg_query*> parts;
  std::vector<int64_t> part_off;
  bool gathered = false;
  // a query over a part of an owner-computes build (kmhg_query_run_device_part): the first row
  // of each query tile (TILE windows from w0), for the root's merge of the parts' rows
  DBuf<uint64_t> tile_off;
  int64_t n_tiles = 0;
  // a range query run for the sharded gather (kmhg_query_run_device_range_runs): its rows as
  // n_runs diagonal runs {first row, i, j} instead of `rows` (n_runs = -1: it holds rows)
  DBuf<int32_t> runs;
  int64_t n_runs = -1;
};

// reads.kmer.pos: the (read, strand, i, j) rows of a batch of reads (kmhg_readsq.h), with what a
// vote over them needs.
struct kmhg_rquery {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t H = 0;
  int64_t n_reads = 0;
  int k = 0;
  DBuf<int32_t> rows;            // 4 per row
};

// seq.kmer.segs: the {i, j, len} segments of some rows (kmhg_rows_segments), complete when the
// handle is returned; `stream` is the stream they were made on.
struct kmhg_segs {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t S = 0;
  DBuf<int32_t> segs;
};

// seq.kmer.blocks: the {i, j, span, hits} blocks of some rows (kmhg_rows_blocks), complete when
// the handle is returned; `stream` is the stream they were made on.
struct kmhg_blocks {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t B = 0;
  DBuf<int32_t> blocks;
};

// seq.kmer.chains: the {i, j, i.end, j.end, hits, blocks} chains of B blocks and chain[b], the
// 1-based chain of every block (kmhg_blocks_chains), complete when the handle is returned;
// `blocks` holds the blocks themselves where the handle made them (kmhg_chains_run*).
struct kmhg_chains {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t C = 0, B = 0;
  DBuf<int32_t> chains, member, blocks;
  bool holds_blocks = false;
};

namespace {

struct DeviceGuard {
  int prev = 0;
  explicit DeviceGuard(int dev) {
    HIPC(hipGetDevice(&prev));
    if (dev != prev) HIPC(hipSetDevice(dev));
  }
  ~DeviceGuard() { (void)hipSetDevice(prev); }
};

inline bool LCN(char c) { return (c | 0x20) == 'n'; }   // LC(c) == 'n', src/kmer_util.h:10

// A host string to the device, returning its C length (its first NUL, else L).  From
// H2D_SCAN_MIN bytes on, a second thread issues the copy of all L bytes while this one scans
// for the NUL (10 MB: 0.07 ms; 500 MB: ~3.5 ms), so the scan costs nothing beside the copy;
// bytes past a NUL are copied and never read.  d_dst holds at least L bytes.
constexpr size_t H2D_SCAN_MIN = 4u << 20;
size_t h2d_cstring(void* d_dst, const char* seq, size_t L, hipStream_t s) {
  if (L < H2D_SCAN_MIN) {
    const size_t n = effective_len(seq, L);
    h2d_host(d_dst, seq, n, s);
    return n;
  }
  int dev = 0;
  HIPC(hipGetDevice(&dev));
  Error err{KMHG_OK, ""};
  std::thread copy([&] {
    try {
      DeviceGuard g(dev);                    // (the current device is per thread)
      h2d_host(d_dst, seq, L, s);
    } catch (const Error& e) {
      err = e;
    }
  });
  const size_t n = effective_len(seq, L);
  copy.join();
  if (err.code != KMHG_OK) fail(err.code, err.msg);
  return n;
}

void check_build_args(size_t L, int k) {
  // make_kmer_h_index, src/kmer_hash.c:514-520
  if (k < 1 || k > 32) fail(KMHG_EINVAL, "k must be a positive integer less than 1+MAX_K");
  if ((int64_t)L <= k) fail(KMHG_EINVAL, "the length of the sequence must be at least k");
  if (L >= (size_t)INT32_MAX) fail(KMHG_EOVERFLOW, "sequence longer than 2^31-1 (int positions)");
}

// A query call (kmhg_querycall.h) that was not refused.
QueryCall checked(const QueryCall& c) {
  if (c.code != KMHG_OK) fail(c.code, c.text);
  return c;
}

void check_query_args(size_t L, int k) { checked(query_call(L, k)); }

// A query entry's call: not refused, and with the index's occurrence cap as it stands now.
QueryCall capped(const kmhg_index* idx, const QueryCall& c);

// fn(i) for every part i, one host thread per distinct key[i] (the first key's on the caller's);
// the parts of one key run in order on its thread.  Every part's failure is kept and the first
// one by part is returned (code KMHG_OK: none), so a caller can release what the others made.
template <class F>
Error for_parts(const std::vector<int>& key, F&& fn) {
  const int n = (int)key.size();
  std::vector<Error> errs(n, Error{KMHG_OK, ""});
  std::vector<int> uniq;
  for (int d : key)
    if (std::find(uniq.begin(), uniq.end(), d) == uniq.end()) uniq.push_back(d);
  auto run_key = [&](int d) {
    for (int i = 0; i < n; ++i) {
      if (key[i] != d) continue;
      try {
        fn(i);
      } catch (const Error& e) {
        errs[i] = e;
      } catch (const std::bad_alloc&) {
        errs[i] = Error{KMHG_ENOMEM, "host allocation failed"};
      }
    }
  };
  std::vector<std::thread> th;
  for (size_t u = 1; u < uniq.size(); ++u) th.emplace_back(run_key, uniq[u]);
  if (!uniq.empty()) run_key(uniq[0]);
  for (auto& t : th) t.join();
  for (const Error& e : errs)
    if (e.code != KMHG_OK) return e;
  return Error{KMHG_OK, ""};
}

// ---------------------------------------------------------------------------- build
kmhg_index* build_device_v1(const uint8_t* d_seq, int64_t L, int k, hipStream_t s) {
  ReleaseGroup rg(s);
  auto idx = std::make_unique<kmhg_index>();
  idx->stream = s;
  idx->build_kind = KMHG_BUILD_GLOBAL;
  HIPC(hipGetDevice(&idx->device));
  idx->k = k;
  idx->L = L;
  const int64_t Nw = L - k + 1;
  const bool aligned = (reinterpret_cast<uintptr_t>(d_seq) & 15) == 0;
  idx->geom = Geom{1u, (uint32_t)table_capacity(Nw)};
  const uint64_t nslots = idx->slots();
  idx->table.reset(nslots);
  DBuf<uint32_t> win_slot(Nw, s);
  LAUNCH("k_table_init", s, launch_table_init(idx->table.p, nslots, s));
  LAUNCH("k_build_insert", s,
         launch_build_insert(d_seq, L, k, idx->table.p, idx->geom, win_slot.p, Nw, aligned, s));
  // compaction scratch: look-back status + ticket + meta in one zeroed block
  const uint32_t nt = tiles_for(nslots);
  const size_t scratch_bytes = (size_t)nt * 8 + 64 + sizeof(BuildMeta);
  DBuf<uint8_t> scratch(scratch_bytes, s);
  HIPC(hipMemsetAsync(scratch.p, 0, scratch_bytes, s));
  uint64_t* status = reinterpret_cast<uint64_t*>(scratch.p);
  uint32_t* ticket = reinterpret_cast<uint32_t*>(scratch.p + (size_t)nt * 8);
  BuildMeta* meta = reinterpret_cast<BuildMeta*>(scratch.p + (size_t)nt * 8 + 64);
  DBuf<uint64_t> ukeys(Nw, s);            // dense CSR arrays: sort bookkeeping only
  DBuf<uint32_t> counts(Nw, s), offsets(Nw + 1, s);
  DBuf<uint32_t> small_ids(Nw / 2 + 1, s), large_ids(Nw / LARGE_MIN + 1, s);
  LAUNCH("k_build_compact", s,
         launch_build_compact(idx->table.p, nslots, status, ticket, ukeys.p, counts.p,
                              offsets.p, small_ids.p, large_ids.p, meta, s));
  idx->positions.reset(Nw);
  LAUNCH("k_build_scatter", s, launch_build_scatter(win_slot.p, Nw, idx->table.p,
                                                    idx->positions.p, s));
  LAUNCH("k_sort_small", s, launch_sort_small(small_ids.p, meta, counts.p, offsets.p,
                                              idx->positions.p, s));
  LAUNCH("k_sort_large", s,
         launch_sort_large(large_ids.p, meta, counts.p, offsets.p, idx->positions.p,
                           reinterpret_cast<int32_t*>(win_slot.p), s));
  LAUNCH("k_inline_singles", s, launch_inline_singles(idx->table.p, nslots, idx->positions.p, s));
  BuildMeta hm;
  HIPC(hipMemcpyAsync(&hm, meta, sizeof(hm), hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  idx->U = hm.n_kmers;
  idx->N = hm.n_positions;
  idx->P = hm.n_pairs;
  idx->max_n = hm.max_count;
  return idx.release();
}

// The partitioned build's switches, once per build: the defaults in the product library, the
// environment's in the test build.  The only place these names are read.
BuildKnobs read_build_knobs() {
  BuildKnobs kn;
  for (const char* name : BUILD_KNOB_NAMES)
    if (const char* v = test_build_knob(name)) set_build_knob(kn, name, v);
  return kn;
}

// One round of the bucket kernel on the current device: its CUs x the workgroups one CU holds
// (cached per device; 0 if the device cannot be queried).
uint32_t bucket_round_of_current_device() {
  static std::atomic<uint32_t> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 0;
  if (dev < 64) {
    if (uint32_t v = cache[dev].load(std::memory_order_relaxed)) return v;
  }
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    cus = 0;
  const uint32_t v = (uint32_t)std::max(cus, 0) * (uint32_t)KMHG_BUCKET_WGS;
  if (dev < 64) cache[dev].store(v, std::memory_order_relaxed);
  return v;
}

// Partitioned build (kmhg_build_v2.hip): LSD radix partition of the windows by hash bucket,
// then one wave per bucket builds its sub-table in LDS.  Falls back to v1 if a bucket's LDS
// sub-table overflows (position builds: never observed -- distinct keys per bucket ~ Binomial,
// mean <= V2_BW; count-only builds retry at spread 1 instead, sh_count_reads_device).
// What is built is a BuildRequest (kmhg_plan.h: the windows of a sequence, a part of them, a key
// stream, a count-only key stream); every decision is plan_build's, and build_device_v2 below
// allocates from the plan and launches.
// Pass A by placement in the bucket kernel (kmhg_build_v2.hip): on unless KMHG_BUCKET_PLACE=0
// (test build) forces the CAS pass everywhere.  The test build also counts, per device buffer
// made once and kept, the buckets placed / fallen back for a repeated key / fallen back for a
// second wrap (kmhg_bucket_place_counters); the product library passes no counters.
#ifdef KMHG_TEST_BUILD
static std::mutex g_place_mu;
static uint32_t* g_place_ctr = nullptr;              // 3 x u32 on g_place_dev
static int g_place_dev = -1;
uint32_t* bucket_place_counters() {
  std::lock_guard<std::mutex> lk(g_place_mu);
  int dev = 0;
  HIPC(hipGetDevice(&dev));
  if (!g_place_ctr) {
    HIPC(hipMalloc(&g_place_ctr, 3 * sizeof(uint32_t)));
    HIPC(hipMemset(g_place_ctr, 0, 3 * sizeof(uint32_t)));
    g_place_dev = dev;
  }
  return dev == g_place_dev ? g_place_ctr : nullptr;
}
#else
uint32_t* bucket_place_counters() { return nullptr; }
#endif

// Which middle stream the bucket-id builds took (test build, kmhg_bid_pack_counters): [0] the
// digit-pos words, [1] every other bucket-id build (the two arrays).  Host counters: the choice is
// made here, not on the device.
#ifdef KMHG_TEST_BUILD
static std::atomic<uint64_t> g_bid_pack_ctr[2];
void count_bid_pack(bool packed) { g_bid_pack_ctr[packed ? 0 : 1].fetch_add(1, std::memory_order_relaxed); }
#else
void count_bid_pack(bool) {}
#endif

// the device buffers a BuildRequest speaks of: the sequence (16-B alignment not required), or
// the key stream
struct StreamPtrs {
  const uint8_t* d_seq = nullptr;
  const uint64_t* d_keys = nullptr;
  const uint32_t* d_mask = nullptr;   // a sampled build's selection mask of d_seq (rq.w > 1)
};

kmhg_index* build_device_v2(const BuildRequest& rq, const StreamPtrs& in, hipStream_t s) {
  ReleaseGroup rg(s);             // the scratch buffers below: one release event
  // Every buffer of the build, the index's own included, is first touched by a kernel, memset or
  // copy queued on s: a build queued behind another on one stream takes over its blocks while
  // that one still runs, with no host wait in between.
  const FirstUseOn on{s};
  const BuildKnobs kn = read_build_knobs();
  const BuildPlan P = plan_build(rq, kn, bucket_round_of_current_device());
  if (P.err != KMHG_OK) fail(P.err, P.msg);
  auto idx = std::make_unique<kmhg_index>();
  idx->stream = s;
  HIPC(hipGetDevice(&idx->device));
  idx->build_kind = ballot_ranks() ? KMHG_BUILD_PARTITIONED_BALLOT : KMHG_BUILD_PARTITIONED;
  idx->k = rq.k;
  idx->L = rq.L;
  idx->is_part = P.is_part;
  idx->geom = P.geom;
  if (P.empty_part) {             // nothing to build
    idx->table.reset(1);
    idx->positions.reset(1);
    return idx.release();
  }
  const int k = rq.k;
  const int64_t L = rq.L, Nw = P.Nw;
  const bool from_keys = P.from_keys, co_auto = P.co_auto, bid = P.bid, partc = P.partc;
  const uint32_t passes = P.passes, R = P.R, ntiles = P.ntiles, nb = P.geom.nb;
  const uint64_t nhist = P.nhist;
  const Geom g = P.geom;
  // every digit of this build: the 32-bit form where the plan allows it
  auto mk_digit = [&](uint32_t dv, uint32_t r) { return make_digit(dv, r, P.digit32 ? g.nb : 0u); };
  const uint64_t* d_keys = in.d_keys;
  // the partition kernels read the sequence as aligned 16-B words: copy an unaligned input
  const uint8_t* d_seq = in.d_seq;
  DBuf<uint8_t> aligned_copy;
  if (!from_keys && (reinterpret_cast<uintptr_t>(d_seq) & 15) != 0) {
    aligned_copy.reset((size_t)L, on);
    HIPC(hipMemcpyAsync(aligned_copy.p, d_seq, (size_t)L, hipMemcpyDeviceToDevice, s));
    d_seq = aligned_copy.p;
  }
  if (bid) count_bid_pack(P.bid_pack);
  // two (first array, position array) buffer pairs, stream p on side P.side(p), each side as
  // wide as the plan says (+ pad)
  auto kwords = [&](int sd) { return ((uint64_t)(Nw + PTILE) * P.key_bytes[sd] + 7) / 8; };
  DBuf<uint64_t> kA(kwords(0), on), kB(kwords(1), on);
  DBuf<uint32_t> pA(P.pos_array[0] ? Nw + PTILE : 1, on), pB(P.pos_array[1] ? Nw + PTILE : 1, on);
  auto kptr = [&](int p) -> void* {
    return p < 0 && from_keys ? const_cast<uint64_t*>(d_keys) : P.side(p) ? kB.p : kA.p;
  };
  auto pptr = [&](int p) { return P.side(p) ? pB.p : pA.p; };
  const uint32_t pad = (uint32_t)Nw;
  DBuf<uint32_t> hist(nhist, on);
  DBuf<uint32_t> start((uint64_t)nb + 1, on);
  DBuf<uint32_t> segb(P.pack8 ? (uint64_t)R * (P.nseg8 + 1) : 1, on);
  // one digit buffer: pass p's histogram has read it before pass p rewrites it for pass p + 1
  DBuf<uint16_t> dsb(P.ds_on ? ((uint64_t)Nw + PTILE + 8) / (P.ds8 ? 2 : 1) + 8 : 1, on);
  uint8_t* ds8p = P.ds8 ? reinterpret_cast<uint8_t*>(dsb.p) : nullptr;
  uint16_t* ds16p = P.ds8 ? nullptr : dsb.p;
  const Pack8 pk8{P.pack8 ? P.sh8 : 0, segb.p, P.nseg8, mk_digit(1, R)};
  // scratch (zeroed in-kernel by V_hist0 / V_hist, no memset): [n_valid][meta][scan status]
  const size_t off_meta = 64, off_status = 128;
  const uint32_t n_status = P.scan_tiles + 1;               // look-back words + ticket
  const size_t scratch_bytes = off_status + (size_t)n_status * 8;
  DBuf<uint8_t> scratch(scratch_bytes, on);
  uint8_t* sc = scratch.p;
  uint32_t* n_valid = reinterpret_cast<uint32_t*>(sc);
  BuildMeta* meta = reinterpret_cast<BuildMeta*>(sc + off_meta);
  uint64_t* status = reinterpret_cast<uint64_t*>(sc + off_status);
  idx->rec = PinnedPool::get().take();                     // V_stats writes the totals here
  if (!co_auto) idx->table.reset(idx->slots(), on);
  idx->sampling = rq.w;
  idx->positions.reset(P.no_pos ? 1 : P.sampled ? std::max<int64_t>(1, rq.n_selected) : Nw, on);
  idx->bstats.reset(nb, on);          // kept: a batch index's walk takes its row offsets from it
  // co_auto: HLL rows of the first histogram pass, V_hll's registers + ticket, its pinned record
  DBuf<uint32_t> hll_rows(co_auto ? (size_t)ntiles * (HLL_REGS / 4) : 1, on);
  DBuf<uint32_t> hll_regs(co_auto ? HLL_PART_WORDS : 1, on);
  PinnedRec hrec;
  if (co_auto) hrec = PinnedPool::get().take();

  // bucket starts straight from the histograms (V_bounds_lo), one level per pass p >= 1:
  // lo_save = pass 0's digit starts (saved by pass 1's V_hist), lvA / lvB = S_p of the passes
  // before the last (3+ passes), the last level writes `start`
  DBuf<uint32_t> lo_save(passes >= 2 ? R : 1, on);
  uint64_t r_top = 1;                                   // R^(passes - 1)
  for (uint32_t i = 1; i < passes; ++i) r_top *= R;
  DBuf<uint32_t> lvA(passes >= 3 ? r_top + 1 : 1, on), lvB(passes >= 4 ? r_top + 1 : 1, on);
  uint32_t div = 1;
  DiagBlock db{nullptr, nullptr, nullptr};
  DBuf<uint32_t> tcnt(partc ? ntiles : 1, on);
  if (from_keys) {   // pass 0 reads the caller's key stream in place (positions implicit)
    HIPC(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(n_valid), (int)Nw, 1, s));
    HIPC(hipMemsetAsync(meta, 0, sizeof(BuildMeta), s));
  } else {
    // a position index keeps its sequence's code words + window bits for the diagonal query
    // path (code words + N flags, 0.5 B per window with the first query's bits; V_hist0 writes them)
    if (rq.codes) {
      idx->dcodes.reset(diag_block_words(Nw), on);
      db = idx->diag_block_of();
    }
    if (P.sampled)   // the selected windows, compacted per tile as a part's are
      LAUNCH("k_minimizer_compact", s,
             launch_minimizer_compact(d_seq, L, k, Nw, in.d_mask, kB.p, pB.p, tcnt.p, ntiles,
                                      status, n_status, meta, s));
    else
      LAUNCH("k_v2_hist0", s,
             launch_v2_hist0(d_seq, L, k, Nw, g, mk_digit(1, R), hist.p, ntiles, status,
                             n_status, meta, s, db.code, db.nbit,
                             bid ? static_cast<uint32_t*>(kptr(-1)) : nullptr,
                             partc ? kB.p : nullptr, partc ? pB.p : nullptr,
                             partc ? tcnt.p : nullptr));
    if (partc) {   // tile counts -> tile offsets, the part's window count -> n_valid
      LAUNCH("k_scan_u32", s, launch_scan_u32(tcnt.p, ntiles, status, n_valid, s));
    } else {       // pass 0: over the sequence, or over V_hist0's ids
      LAUNCH("k_scan_u32", s, launch_scan_u32(hist.p, nhist, status, n_valid, s));
      const DigitOut ds0{ds16p, mk_digit(R, R), ds8p};
      LAUNCH("k_v2_scatter_seq", s,
             launch_v2_scatter(bid ? ScatterIn::first_pass(kptr(-1), Nw)
                                   : ScatterIn::sequence(d_seq, L, k, Nw),
                               P.F(-1), P.F(0), kptr(0), pptr(0), pad, n_valid, g, mk_digit(1, R),
                               hist.p, ntiles, s, nullptr, P.pack8 ? &pk8 : nullptr,
                               P.ds_out(0) ? &ds0 : nullptr));
      // the segment table, before pass 1's histogram overwrites pass 0's
      if (P.pack8)
        LAUNCH("k_seg_bounds", s,
               launch_seg_bounds(hist.p, ntiles, R, P.nseg8, (uint32_t)(P.seg8 / PTILE), n_valid,
                                 segb.p, s));
      div = R;
    }
  }
  // the later passes' histogram layout: [digit][tile] over the tiles of their input.  A part
  // build keeps ~1/n_parts of the windows after pass 0, so it reads that count back and sizes
  // the later passes to it (a separate histogram, so pass 0's column 0 stays readable) instead
  // of walking every window's tile again -- one host round trip per part build.
  uint32_t* hp = hist.p;
  uint32_t C = ntiles, nst = n_status;
  uint64_t nh = nhist;
  DBuf<uint32_t> hist1;
  if ((rq.n_parts >= 2 && (passes > 1 || partc)) || P.sampled) {
    uint32_t nv = (uint32_t)rq.n_selected;   // a sampled build knows its count already
    if (!P.sampled) {
      HIPC(hipMemcpyAsync(&nv, n_valid, 4, hipMemcpyDeviceToHost, s));
      HIPC(hipStreamSynchronize(s));
    }
    C = std::max<uint32_t>(1u, (uint32_t)(((uint64_t)nv + PTILE - 1) / PTILE));
    nh = (uint64_t)R * C;
    nst = tiles_for(nh) + 1;
    hist1.reset(nh, on);
    hp = hist1.p;
    // pass 0's digit starts (its scanned column 0), which pass 1's V_hist saves otherwise
    if (!partc)
      HIPC(hipMemcpy2DAsync(lo_save.p, 4, hist.p, (size_t)ntiles * 4, 4, R,
                            hipMemcpyDeviceToDevice, s));
  }
  if (partc)   // the part's windows, dense in window order: every radix pass reads these
    LAUNCH("k_part_dense", s, launch_part_dense(kB.p, pB.p, tcnt.p, ntiles, n_valid, kptr(-1),
                                                pptr(-1), P.F(-1), s));
  // where pass 1 saves column 0: pass 0's histogram is hp's unless pass 0 was the one over
  // every window (its own layout, copied above)
  uint32_t* save1 = hp == hist.p || partc ? lo_save.p : nullptr;
  // each level of the bucket starts rides in its pass (BoundsFuse) where the plan fused it
  auto level_of = [&](uint32_t p, uint32_t spread) {
    uint64_t dv = 1;                                    // R^p lower-digit values
    for (uint32_t i = 0; i < p; ++i) dv *= R;
    const bool last = p + 1 == passes;
    const uint32_t* lin = p == 1 ? lo_save.p : ((p - 1) % 2 ? lvA.p : lvB.p);
    uint32_t* lout = last ? start.p : (p % 2 ? lvA.p : lvB.p);
    return BoundsFuse{lin, lout, mk_digit((uint32_t)dv, R), (uint32_t)dv, spread,
                      last ? g.nb : (uint32_t)(dv * R)};
  };
  auto launch_level = [&](uint32_t p, const BoundsFuse& f) {   // over pass p's input
    LAUNCH("k_v2_bounds", s,
           launch_v2_bounds_lo(P.F((int)p - 1), kptr((int)p - 1), n_valid, g, f.Dlast, f.div, hp, C,
                               f.lo_start, f.spread, f.start, f.nlim, s, pk8.sh));
  };
  // the radix passes left: histogram (of the digits the pass before left, else of its input),
  // scan, scatter with the fused level, the level on its own where it is not fused
  for (uint32_t p = P.first_pass; p < passes; ++p) {
    const Digit Dp = mk_digit(div, R);
    const bool keys0 = from_keys && p == 0;
    const bool last = p + 1 == passes;
    const bool hll = co_auto && p == 0;
    const int pi = (int)p - 1;                          // the pass's input stream
    if (keys0)
      LAUNCH("k_v2_hist", s,
             launch_v2_hist_keys0(d_keys, n_valid, g, Dp, hp, C, status, nst, s,
                                  hll ? hll_rows.p : nullptr, hll ? hll_regs.p : nullptr,
                                  rq.skip_empty));
    else
      LAUNCH("k_v2_hist", s,
             launch_v2_hist(!P.ds_out(pi) ? P.F(pi)
                            : P.ds8       ? StreamFmt::Digits8
                                          : StreamFmt::Digits16,
                            P.ds_out(pi) ? dsb.p : kptr(pi), n_valid, g, Dp, hp, C, status, nst, s,
                            p == 1 ? save1 : nullptr, pk8.sh));
    LAUNCH("k_scan_u32", s, launch_scan_u32(hp, nh, status, n_valid, s));
    if (hll) {   // after the scan: the estimate travels with the valid key count
      LAUNCH("k_v2_hll", s, launch_v2_hll(hll_rows.p, ntiles, hll_regs.p,
                                          &hrec.meta->distinct_est, n_valid,
                                          &hrec.meta->n_positions, s));
      // a pinned record's event keeps its system-scope fence: the host reads the estimate
      // through it below, mid-build
      HIPC(hipEventRecord(hrec.ev, s));
    }
    const BoundsFuse lv = level_of(p, 1u);              // (pass 0 has none: never fused)
    const DigitOut dsn{ds16p, mk_digit(div * R, R), ds8p};
    LAUNCH("k_v2_scatter", s,
           launch_v2_scatter(keys0 ? ScatterIn::first_pass(d_keys, Nw, rq.skip_empty)
                                   : ScatterIn::stream(kptr(pi), pptr(pi)),
                             P.F(pi), P.F((int)p), kptr((int)p), pptr((int)p), pad, n_valid, g, Dp,
                             hp, C, s, P.fused(p) ? &lv : nullptr, P.pack8 ? &pk8 : nullptr,
                             P.ds_out((int)p) ? &dsn : nullptr));
    if (p >= 1 && !P.fused(p) && !last) launch_level(p, lv);
    div *= R;
  }
  const int last_p = (int)passes - 1;   // its stream is the bucket kernel's
  Geom gb = g;                     // the bucket stage's geometry
  if (co_auto) {
    // the estimate landed while the later radix passes were still queued on the device
    HIPC(hipEventSynchronize(hrec.ev));
    idx->co_est = hrec.meta->distinct_est;
    const uint64_t n_keys_valid = hrec.meta->n_positions;
    PinnedPool::get().give(hrec, false);
    idx->co_spread = co_spread_for(idx->co_est, n_keys_valid, kn.co_spread);
    gb = Geom{nb / (uint32_t)idx->co_spread, V2_CAPW};
    idx->geom = gb;
    idx->table.reset(idx->slots(), on);
  }
  if (passes == 1) {
    // one pass (pass 0 reads chars or the caller's keys): the starts are the scanned column 0
    LAUNCH("k_v2_bounds", s,
           launch_v2_bounds_lo(StreamFmt::Keys, nullptr, n_valid, g, mk_digit(1, R), 1u,
                               partc ? hp : hist.p, partc ? C : ntiles, nullptr, g.nb / gb.nb,
                               start.p, g.nb, s));
  } else if (!P.fused(passes - 1)) {
    launch_level(passes - 1, level_of(passes - 1, g.nb / gb.nb));
  }
#ifdef KMHG_STAMPS
  static uint64_t* stamps = nullptr;
  if (!stamps) HIPC(hipMallocManaged(&stamps, sizeof(uint64_t) * 8 * (1u << 22)));
  HIPC(hipMemsetAsync(stamps, 0, sizeof(uint64_t) * 8 * nb, s));
  kmhg::set_stamp_buffer(stamps);
#endif
  // tests only: a corrupted stream or bound (KMHG_TEST_DISORDER=1|2|3) -> the bucket kernel's
  // checks -> v1 rebuild
  if (kn.test_disorder && !P.no_pos)
    launch_v2_test_disorder(P.F(last_p), kptr(last_p), pptr(last_p), start.p, n_valid,
                            kn.test_disorder, s);
  // Build-time tags (the plan's want_tags): the build writes the diagonal query path's slot
  // tags and repeated-key bits itself
  uint8_t* tg = nullptr;
  uint32_t* rep = nullptr;
  if (P.want_tags) {
    try {
      idx->ptag.reset(idx->slots() + 32, on);    // + the 32-B span the last probe group reads
      tg = idx->ptag.p;
      rep = db.uniq;
      HIPC(hipMemsetAsync(rep, 0, diag_uniq_words(Nw) * 4, s));
      // the side slot's tag (its key is the empty sentinel: 0) and the tail
      HIPC(hipMemsetAsync(tg + idx->slots() - 1, 0, 33, s));
    } catch (const Error& e) {               // no room for the tags: the first query makes them
      if (e.code != KMHG_ENOMEM) throw;
      (void)hipGetLastError();
      tg = nullptr;
      rep = nullptr;
    }
  }
  LAUNCH("k_v2_bucket_wg", s,
         launch_v2_bucket_wg(P.F(last_p), kptr(last_p), pptr(last_p), start.p, gb, idx->table.p,
                             idx->positions.p, idx->bstats.p, meta, s, n_valid, (uint32_t)Nw,
                             db.code, k, tg, rep, kn.bucket_place, bucket_place_counters()));
  idx->tags_built = tg != nullptr;
  LAUNCH("k_v2_stats", s, launch_v2_stats(idx->bstats.p, gb.nb, n_valid, meta, idx->rec.meta, s));
  idx->bstats_nb = gb.nb;
  // the build's one marker: finish_build() waits on it for the totals, and the scratch buffers
  // above wait behind it too (nothing below launches on s).  Every earlier exit, a throw
  // included, leaves the group to record an event of its own.
  HIPC(hipEventRecord(idx->rec.ev, s));
  rg.adopt(idx->rec.ev);
#ifdef KMHG_STAMPS
  if (const char* f = std::getenv("KMHG_STAMP_FILE")) {
    HIPC(hipStreamSynchronize(s));
    if (FILE* fp = fopen(f, "wb")) { fwrite(stamps, 8, 8 * (size_t)nb, fp); fclose(fp); }
  }
#endif
  // no wait here: the build completes in stream order and finish_build() collects the totals
  idx->pending = true;
  idx->src = in.d_seq;             // the caller's buffer (the v1 fallback re-reads it)
  return idx.release();
}

// the tag filter of the diagonal query path (per call: tests switch it)
bool tags_on() {
  const char* e = test_build_knob("KMHG_QUERY_TAGS");
  return !(e && e[0] == '0');
}

// The LDS lane-order property the radix ranks rest on (kmhg_build_v2.hip), checked once per
// device before its first partitioned build: where lanes of one returning LDS add that hit the
// same counter are not served in lane order, every build takes the ballot-rank kernels.
// KMHG_TEST_BALLOT=1 (tests) forces them.
static std::atomic<int> g_lane_state[64];          // 0 unchecked, 1 lane order holds, 2 ballots
static std::mutex g_lane_mu;
// The check's stream and result buffer are made once per device and kept: no hipFree (which
// waits for the whole device, stalling work other streams have in flight) and only the check's
// own stream is synchronized.
static void lane_order_run(int blocks, uint64_t* bad, uint64_t* checked) {
  struct Probe {
    hipStream_t st = nullptr;
    unsigned long long* res = nullptr;
  };
  static Probe probes[64];                         // under g_lane_mu (callers hold it)
  int dev = 0;
  HIPC(hipGetDevice(&dev));
  Probe& pr = probes[(unsigned)dev % 64];
  if (!pr.st) HIPC(hipStreamCreateWithFlags(&pr.st, hipStreamNonBlocking));
  if (!pr.res) HIPC(hipMalloc(&pr.res, 2 * sizeof(unsigned long long)));
  unsigned long long h[2] = {0, 0};
  hipError_t e = hipMemsetAsync(pr.res, 0, sizeof(h), pr.st);
  if (e == hipSuccess) {
    launch_lane_order_check(pr.res, pr.st, blocks);
    e = hipMemcpyAsync(h, pr.res, sizeof(h), hipMemcpyDeviceToHost, pr.st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(pr.st);
  hip_check(e, "LDS lane-order check");
  *bad = h[0];
  *checked = h[1];
}
bool lane_ballot() {
  if (const char* e = test_build_knob("KMHG_TEST_BALLOT"))
    if (e[0] == '1') return true;
  int dev = 0;
  HIPC(hipGetDevice(&dev));
  std::atomic<int>& st = g_lane_state[(unsigned)dev % 64];
  int v = st.load(std::memory_order_acquire);
  if (v == 0) {
    std::lock_guard<std::mutex> lk(g_lane_mu);
    v = st.load(std::memory_order_relaxed);
    if (v == 0) {
      uint64_t bad = 0, chk = 0;
      lane_order_run(256, &bad, &chk);
      v = (bad == 0 && chk > 0) ? 1 : 2;
      st.store(v, std::memory_order_release);
    }
  }
  return v == 2;
}

int build_version() {   // read per build so tests can exercise the fallback (KMHG_BUILD=v1)
  const char* e = test_build_knob("KMHG_BUILD");
  return (e && std::string(e) == "v1") ? 1 : 2;
}

// Returns a possibly pending index (partitioned build); finish_build() completes it.
// codes: keep the sequence's code words for the diagonal query path (position indices; a
// count.kmers batch index has no use for them)
kmhg_index* build_device(const uint8_t* d_seq, int64_t L, int k, hipStream_t s, bool codes = true) {
  if (const char* e = test_build_knob("KMHG_DIAG_CODES"))   // tests / A/B: no code block
    if (e[0] == '0') codes = false;
  if (build_version() == 2)
    return build_device_v2(BuildRequest::sequence(L, k, codes), StreamPtrs{d_seq, nullptr}, s);
  return build_device_v1(d_seq, L, k, s);
}

// The selection mask of a strand of d_seq at (k, w) into d_mask (minimizer_mask_words words);
// returns the number selected (one wait on s: the count sizes what follows).
int64_t minimizer_mask_device(const uint8_t* d_seq, int64_t L, int k, int w, bool rc,
                              uint32_t* d_mask, hipStream_t s) {
  const bool aligned = (reinterpret_cast<uintptr_t>(d_seq) & 15) == 0;
  DBuf<unsigned long long> total(1, s);
  HIPC(hipMemsetAsync(total.p, 0, sizeof(unsigned long long), s));
  LAUNCH("k_minimizer_mask", s,
         launch_minimizer_mask(d_seq, L, k, w, rc, aligned, d_mask, total.p, s));
  unsigned long long n = 0;
  HIPC(hipMemcpyAsync(&n, total.p, sizeof(n), hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  return (int64_t)n;
}

void check_sampling_args(int k, int64_t w) {
  if (const char* bad = minimizer_w_refusal(w)) fail(KMHG_EINVAL, bad);
  if (w > 1 && k > 31) fail(KMHG_EINVAL, "a sampled index needs k <= 31");
}

// kmhg_build_sampled*: w = 1 is build_device itself; w > 1 selects first (one wait: the count
// sizes the table), then builds the selected windows with the partitioned build.  The
// global-atomic build does not sample.
kmhg_index* build_device_sampled(const uint8_t* d_seq, int64_t L, int k, int w, hipStream_t s) {
  if (w == 1) return build_device(d_seq, L, k, s);
  if (build_version() != 2) fail(KMHG_EINVAL, "a sampled index needs the partitioned build");
  ReleaseGroup rg(s);
  DBuf<uint32_t> mask((size_t)minimizer_mask_words(L - k + 1), s);
  const int64_t n_sel = minimizer_mask_device(d_seq, L, k, w, false, mask.p, s);
  return build_device_v2(BuildRequest::sequence_sampled(L, k, w, n_sel),
                         StreamPtrs{d_seq, nullptr, mask.p}, s);
}

// Wait for a pending build and collect its totals.  If a bucket's LDS sub-table overflowed
// (position builds: never observed -- distinct keys per bucket ~ Binomial with mean <= V2_BW;
// count-only builds do not come here), the index is rebuilt
// with the global-atomic build from the retained input.
void finish_build(kmhg_index* idx) {
  if (!idx->pending) return;
  HIPC(hipEventSynchronize(idx->rec.ev));
  const BuildMeta hm = *idx->rec.meta;
  PinnedPool::get().give(idx->rec, false);
  idx->rec = PinnedRec{};
  idx->pending = false;
  const uint8_t* src = idx->src;
  idx->src = nullptr;
  if (hm.overflow) {
    if (idx->sampling > 1)
      fail(KMHG_EOVERFLOW, "a bucket of a sampled build overflowed its LDS table (the global-atomic "
                           "build does not sample)");
    if (idx->is_part) fail(KMHG_EOVERFLOW, "a bucket of a part build overflowed its LDS table");
    std::unique_ptr<kmhg_index> v1(build_device_v1(src, idx->L, idx->k, idx->stream));
    idx->build_kind = KMHG_BUILD_GLOBAL;
    idx->tags_built = false;                     // the tags were the partitioned table's
    idx->bstats_nb = 0;                          // one global bucket: no per-bucket statistics
    idx->fallback = 1;                      // reported by kmhg_index_info (bench.py fails on it)
    idx->geom = v1->geom;
    idx->table.swap_with(v1->table);
    idx->positions.swap_with(v1->positions);
    idx->U = v1->U; idx->N = v1->N; idx->P = v1->P; idx->max_n = v1->max_n;
    v1->table.bind(idx->stream);
    v1->positions.bind(idx->stream);
    return;
  }
  idx->U = hm.n_kmers;
  idx->N = hm.n_positions;
  idx->P = hm.n_pairs;
  idx->max_n = hm.max_count;
}

// ---------------------------------------------------------------------------- query
// The diagonal path's once-per-index preparation (DiagIdx, kmhg_kernels.h): the uniq bits of
// the windows of repeated keys, and the slot tags where the build did not write them.  True when
// the path may be used: prepared now, or by an earlier query, possibly on another thread.  One
// synchronize, once per index: later queries may run on other streams.  Without room for the
// tags the index stays on table probes for good (ps_failed).
bool ensure_diag(kmhg_index* idx, hipStream_t s) {
  if (idx->ps_ready.load(std::memory_order_acquire)) return true;
  std::lock_guard<std::mutex> lk(idx->ps_mu);
  if (idx->ps_ready.load(std::memory_order_relaxed) || idx->ps_failed) return !idx->ps_failed;
  if (!idx->tags_built) {
    try {
      idx->ptag.reset(idx->slots() + 32);  // + the 32-B span the last probe group reads
    } catch (const Error& e) {             // no room for the tags: table probes only
      if (e.code != KMHG_ENOMEM) throw;
      idx->ps_failed = true;
      (void)hipGetLastError();
      return false;
    }
    idx->ptag.bind(s);
  }
  idx->dcodes.bind(s);
  const DiagBlock db = idx->diag_block_of();
  if (idx->tags_built)                     // the build wrote the tags and repeat bits
    LAUNCH("k_diag_valid", s, launch_diag_valid(db.nbit, idx->L, idx->k, db.uniq, true, s));
  else
    LAUNCH("k_diag_prep", s,
           launch_diag_prep(db.nbit, idx->L, idx->k, db.uniq, idx->table.p, idx->slots(),
                            idx->positions.p, idx->ptag.p, s));
  HIPC(hipStreamSynchronize(s));
  idx->ps_ready.store(true, std::memory_order_release);
  return true;
}

QueryCall capped(const kmhg_index* idx, const QueryCall& c) {
  return checked(c)
      .with_max_occ(idx->max_occ.load(std::memory_order_relaxed))
      .with_sampling(c.k == idx->k ? idx->sampling : 1);
}

// The occurrence cap on a probed query's records, before their tile totals are scanned
// (k_qrec_mask); nothing is launched without a cap.
// A sampled index (c.sampling > 1) first drops the records of the query windows its rule does
// not select: the rule runs over the whole strand of c.L chars (k_minimizer_mask), the records
// of windows [c.w0, c.w1) are masked (k_qrec_minmask).  Both are per-window drops: the result is
// their intersection.
void mask_records(const QueryCall& c, const uint8_t* d_seq, uint32_t* qrec, const uint2* qmulti,
                  uint64_t* tile_rows, hipStream_t s) {
  if (c.sampling > 1) {
    const bool aligned = (reinterpret_cast<uintptr_t>(d_seq) & 15) == 0;
    DBuf<uint32_t> mask((size_t)minimizer_mask_words(c.L - c.k + 1), s);
    DBuf<unsigned long long> total(1, s);
    HIPC(hipMemsetAsync(total.p, 0, sizeof(unsigned long long), s));
    LAUNCH("k_minimizer_mask", s,
           launch_minimizer_mask(d_seq, c.L, c.k, c.sampling, c.rc, aligned, mask.p, total.p, s));
    LAUNCH("k_qrec_minmask", s,
           launch_qrec_minmask(qrec, qmulti, c.w1 - c.w0, c.w0, mask.p, tile_rows, s));
  }
  if (c.max_occ == 0) return;
  LAUNCH("k_qrec_mask", s,
         launch_qrec_mask(qrec, qmulti, c.w1 - c.w0, (uint32_t)c.max_occ, tile_rows, s));
}

// Windows [c.w0, c.w1) of the query.  Rows come out ordered by window end, so shards of
// consecutive window ranges concatenate to the unsharded result.
// c.rc: the reverse strand (kmhg_query_run_rc*).  d_seq is still the FORWARD sequence; only the
// probe's stage fill differs, and w0, w1 and the rows' i are in rc(seq)'s coordinates.
kmhg_query* query_device(kmhg_index* idx, const uint8_t* d_seq, const QueryCall& c,
                         hipStream_t s) {
  ReleaseGroup rg(s);
  if (idx->canonical) fail(KMHG_EINVAL, "External pointer has incorrect tag");
  if (idx->is_part != c.part)
    fail(KMHG_EINVAL, idx->is_part ? "a part index must be assembled before it is queried"
                                   : "not a part of an owner-computes build");
  finish_build(idx);
  auto q = std::make_unique<kmhg_query>();
  q->device = idx->device;
  q->stream = s;
  idx->stream = s;
  const int64_t L = c.L, w0 = c.w0, w1 = c.w1, Nw = w1 - w0;
  const int kq = c.k;
  if (Nw <= 0) return q.release();
  const bool aligned = (reinterpret_cast<uintptr_t>(d_seq) & 15) == 0;
  const uint32_t nt = tiles_for(Nw);
  uint64_t cap = query_rows_guess(Nw);
  if (!c.runs) q->rows.reset(cap);
  // probe / scan / emit.  (A one-pass probe + look-back + emit was measured slower and removed
  // in round 4: config 2 0.403 against 0.365 ms; re-measured round 3 with the diagonal path,
  // self query 94 -> 53 Gbp/s -- a tile that has probed waits for its predecessors' totals
  // while holding its CU slot, and the probe is occupancy / latency bound.)
  uint64_t H = 0;
  // (a part query too: its anchors and verified windows count only where the part owns the key,
  // and its tags and repeated-key bits come from its own table, k_query_probe<..., PART>)
  const char* de = test_build_knob("KMHG_QUERY_DIAG");
  const bool diag = diag_eligible(kq, idx->k, idx->sources, idx->L - idx->k + 1, idx->U,
                                  idx->dcodes.p != nullptr, !(de && de[0] == '0'), idx->sampling) &&
                    ensure_diag(idx, s);

  DBuf<uint32_t> qrec(Nw, s);         // per window: 0, the one hit's position, or multi
  DBuf<uint2> qmulti(Nw, s);          // {count, first index}: written for multi-hit windows only
  // per-tile rows -> first row; then the long-scan scratch.  The row total goes straight into
  // pinned host memory (no copy launch before the host reads it).
  DBuf<uint64_t> tiles((size_t)nt + scan_u64_scratch(nt), s);
  uint64_t* tile_row0 = tiles.p;
  DBuf<uint32_t> elist((size_t)nt + 1, s);   // tiles with a multi-hit window; [nt] = their count
  PinnedRec hrec = PinnedPool::get().take();
  GiveBack give_back{hrec, s};
  uint64_t* total = &hrec.meta->n_kmers;
  LAUNCH("k_query_probe", s,
         launch_query_probe(d_seq, L, kq, idx->table.p, idx->geom, qrec.p, qmulti.p, w0, w1, aligned,
                            tile_row0, s, diag ? idx->diag_view() : DiagIdx{nullptr, nullptr, 0},
                            diag && tags_on() ? idx->ptag.p : nullptr, elist.p + nt, c.rc));
  mask_records(c, d_seq, qrec.p, qmulti.p, tile_row0, s);
  LAUNCH("k_scan_tiles_u64", s, launch_scan_u64(tile_row0, nt, total, tiles.p + nt, s));
  if (c.runs) {
    // the rows as diagonal runs, made from the window records (k_qruns_*); rows written only
    // when runs would not be smaller (runs_pay)
    DBuf<uint64_t> rtiles((size_t)nt + scan_u64_scratch(nt), s);
    PinnedRec hrec2 = PinnedPool::get().take();
    GiveBack give_back2{hrec2, s};
    uint64_t* n_runs = &hrec2.meta->n_kmers;
    LAUNCH("k_qruns_count", s, launch_qruns_count(qrec.p, qmulti.p, (uint64_t)Nw, rtiles.p, s));
    LAUNCH("k_scan_tiles_u64", s, launch_scan_u64(rtiles.p, nt, n_runs, rtiles.p + nt, s));
    HIPC(hipStreamSynchronize(s));
    H = __atomic_load_n(total, __ATOMIC_ACQUIRE);
    const uint64_t NR = __atomic_load_n(n_runs, __ATOMIC_ACQUIRE);
    q->H = (int64_t)H;
    if (H > (uint64_t)INT32_MAX) fail(KMHG_EOVERFLOW, "result has more than 2^31-1 rows");
    if (runs_pay(H, NR)) {
      q->runs.reset(3 * NR);
      q->n_runs = (int64_t)NR;
      LAUNCH("k_qruns_emit", s,
             launch_qruns_emit(qrec.p, qmulti.p, idx->positions.p, (uint64_t)Nw, w0, kq,
                               tile_row0, rtiles.p, NR, q->runs.p, s));
      return q.release();
    }
    cap = std::max<uint64_t>(H, 1);              // the rows, into an exact buffer
    q->rows.reset(cap);
  }
  LAUNCH("k_query_emit", s,
         launch_query_emit(qrec.p, qmulti.p, Nw, w0, kq, idx->positions.p, tile_row0, q->rows.p, cap,
                           elist.p, elist.p + nt, true, s));
  HIPC(hipStreamSynchronize(s));
  H = __atomic_load_n(total, __ATOMIC_ACQUIRE);
  q->H = (int64_t)H;
  if (c.part) {                  // the tile offsets stay with the query (the root's merge)
    tiles.bind(s);
    q->tile_off.swap_with(tiles);
    q->n_tiles = nt;
  }
  if (!needs_exact_redo(H, cap)) {
    rg.synced = true;                            // nothing queued behind the synchronize
    return q.release();
  }
  q->rows.bind(s);
  q->rows.reset(H);
  LAUNCH("k_query_emit", s,
         launch_query_emit(qrec.p, qmulti.p, Nw, w0, kq, idx->positions.p, tile_row0, q->rows.p, H,
                           elist.p, elist.p + nt, false, s));
  return q.release();
}

void prepare_readout(kmhg_index* idx, hipStream_t s);

// ---------------------------------------------------------------------------- kmer.pairs
// Rows (a, b) for the k-mers both indices hold, a's k-mers in a's kmer.pos row order
// (kmhg_join.hip).  Same two-phase shape as the query: probe + tile totals, one read-back, emit.
kmhg_query* pairs_device(kmhg_index* a, kmhg_index* b, hipStream_t s) {
  ReleaseGroup rg(s);
  if (a->canonical || b->canonical) fail(KMHG_EINVAL, "External pointer has incorrect tag");
  // (the probe hashes over b's own bucket count and the readout walks a's own slots: a part
  // would answer for the wrong buckets without a word)
  if (a->is_part || b->is_part)
    fail(KMHG_EINVAL, "a part index must be assembled before it is read");
  finish_build(a);
  finish_build(b);
  if (a->k != b->k) fail(KMHG_EINVAL, "the two indices must have the same k");
  if (a->device != b->device) fail(KMHG_EINVAL, "the two indices must be on the same device");
  prepare_readout(a, s);
  auto q = std::make_unique<kmhg_query>();
  q->device = a->device;
  q->stream = s;
  a->stream = s;
  b->stream = s;
  const uint32_t Ua = (uint32_t)a->U;
  if (Ua == 0 || b->U == 0) return q.release();
  const uint32_t nt = tiles_for(Ua);
  DBuf<uint4> jinfo(Ua, s);
  DBuf<uint64_t> tiles((size_t)nt + 1 + scan_u64_scratch(nt), s);
  LAUNCH("k_join_probe", s, launch_join_probe(a->canon.perm.p, Ua, a->table.p, b->table.p, b->geom,
                                              jinfo.p, tiles.p, s));
  LAUNCH("k_scan_tiles_u64", s, launch_scan_u64(tiles.p, nt, tiles.p + nt, tiles.p + nt + 1, s));
  uint64_t H = 0;
  HIPC(hipMemcpyAsync(&H, tiles.p + nt, sizeof(H), hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  q->H = (int64_t)H;
  q->rows.reset(H);
  if (H)
    LAUNCH("k_join_emit", s, launch_join_emit(jinfo.p, Ua, a->positions.p, b->positions.p, tiles.p,
                                              q->rows.p, s));
  return q.release();
}

// ---------------------------------------------------------------------------- count.kmers
void prepare_canon(kmhg_index* idx, hipStream_t s);

// One count.kmers batch (a device-resident sequence) merged into the counts index `idx`
// (kmhg_count.hip): partitioned build of the batch -> its distinct keys in first-occurrence
// order -> probe / append into the count matrix -> table rebuilt for the grown key list.
struct Release {                   // a batch index dies in stream order
  kmhg_index* b; hipStream_t s;
  ~Release() { b->bind_all(s); }
};

void merge_batch(kmhg_index* idx, kmhg_index* B, uint32_t source, uint64_t base, hipStream_t s);

// Room for `need` rows in the count matrix (grown geometrically: repeated calls amortise the copy).
void reserve_rows(kmhg_index* idx, uint64_t need, hipStream_t s) {
  const uint32_t S = idx->sources;
  const uint64_t U0 = idx->U;
  if (need * S > (uint64_t)INT32_MAX)
    fail(KMHG_EOVERFLOW, "counts index larger than 2^31-1 counts (R vector limit)");
  if (need <= idx->rows_cap) return;
  const uint64_t cap = std::max<uint64_t>(need, idx->rows_cap * 2);
  const bool ord = !idx->canonical;               // count.kmers rows carry order keys
  DBuf<uint64_t> nk(cap), nr(ord ? cap : 0);
  DBuf<int32_t> nm(cap * S);
  if (U0) {
    HIPC(hipMemcpyAsync(nk.p, idx->ckeys.p, U0 * 8, hipMemcpyDeviceToDevice, s));
    HIPC(hipMemcpyAsync(nm.p, idx->positions.p, U0 * S * 4, hipMemcpyDeviceToDevice, s));
    if (ord) HIPC(hipMemcpyAsync(nr.p, idx->rord.p, U0 * 8, hipMemcpyDeviceToDevice, s));
  }
  idx->ckeys.bind(s);
  idx->positions.bind(s);
  idx->rord.bind(s);
  idx->ckeys.swap_with(nk);
  idx->positions.swap_with(nm);
  idx->rord.swap_with(nr);
  idx->rows_cap = cap;
}

// The first batch into an empty counts index or suffix hash: every key is new, the batch table
// becomes the counts table, and its occupied slots are compacted into rows in slot order in one
// pass (k_count_walk) -- no probe, append, table rebuild or C_fix.  count.kmers rows get their
// order keys (base + first position - 1); a suffix hash's rows are order-free.  Returns the
// rows written (B->U, exact, when the batch was built from a sequence).
uint64_t adopt_first_batch(kmhg_index* idx, kmhg_index* B, uint32_t source, uint64_t base,
                           hipStream_t s) {
  ReleaseGroup rg(s);
  const uint32_t S = idx->sources;
  const uint64_t Ub = B->U;
  reserve_rows(idx, Ub, s);
  const bool ord = !idx->canonical;
  const uint64_t ns = B->slots();
  idx->table.bind(s);
  idx->slot_row.bind(s);
  idx->row_slot.bind(s);
  idx->geom = B->geom;
  idx->table.swap_with(B->table);                  // B's release frees the old (empty) table
  idx->slot_row.reset(ns);
  idx->row_slot.reset(Ub);
  const int32_t* bpos = ord ? B->positions.p : nullptr;
  uint64_t* rord = ord ? idx->rord.p : nullptr;
  uint64_t n_new = Ub;
  const char* we = test_build_knob("KMHG_COUNT_WALK");   // "lb": the look-back walk (A/B, tests)
  if (B->bstats_nb == B->geom.nb && B->geom.nb > 0 && !(we && std::string(we) == "lb")) {
    // bucket-aligned tiles, row offsets from the bucket statistics: no look-back chain
    const uint32_t nt = count_walk_b_tiles(B->geom.nb);
    const uint32_t st = tiles_for(nt);
    DBuf<uint32_t> tc(nt + 2, s);                  // tile counts -> offsets; [nt] total, [nt+1] err
    DBuf<uint64_t> status((size_t)st + 1, s);
    HIPC(hipMemsetAsync(status.p, 0, ((size_t)st + 1) * 8, s));
    LAUNCH("k_walk_counts", s,
           launch_walk_counts(B->bstats.p, idx->table.p, idx->geom, tc.p, nt, tc.p + nt + 1, s));
    LAUNCH("k_scan_u32", s, launch_scan_u32(tc.p, nt, status.p, tc.p + nt, s));
    LAUNCH("k_count_walk_b", s,
           launch_count_walk_b(idx->table.p, idx->geom, tc.p, nt, S, source, idx->ckeys.p,
                               idx->positions.p, idx->slot_row.p, idx->row_slot.p, bpos, rord,
                               base, tc.p + nt + 1, s));   // tc: offsets, [nt] = total
    uint32_t h[2] = {0, 0};                        // rows written, consistency flag
    HIPC(hipMemcpyAsync(h, tc.p + nt, 8, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    if (h[1]) fail(KMHG_EDEVICE, "counts walk: bucket statistics disagree with the table (internal error)");
    n_new = h[0];
  } else {
    const uint64_t nw = count_walk_tiles(ns);
    DBuf<uint64_t> status(nw + 1, s);              // look-back words + the tile ticket
    HIPC(hipMemsetAsync(status.p, 0, (nw + 1) * 8, s));
    LAUNCH("k_count_walk", s,
           launch_count_walk(idx->table.p, ns, status.p,
                             reinterpret_cast<uint32_t*>(status.p + nw), S, source, idx->ckeys.p,
                             idx->positions.p, idx->slot_row.p, idx->row_slot.p, bpos, rord, base,
                             s));
    uint64_t last = 0;                             // the last tile's inclusive prefix
    HIPC(hipMemcpyAsync(&last, status.p + nw - 1, 8, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    n_new = last & ((1ull << 62) - 1);             // LB_MASK: payload of a status word
  }
  idx->U = n_new;
  idx->N = n_new * S;
  idx->P = n_new * ((uint64_t)S * (S - 1) / 2);
  idx->max_n = n_new ? S : 0;
  idx->kmer_count += n_new;
  idx->order_ready = !ord;
  idx->canon.ready = false;
  return n_new;
}

// Adopting a batch table keeps its size, set by the batch's windows / k-mer words; the rebuild
// sizes the table by the distinct keys (~1.5 slots per key).  A batch with heavy repetition
// (deep read coverage) would leave a sparse, oversized table, so adoption needs <= 6 slots per
// distinct key (<= 4x the rebuilt table); otherwise the general merge rebuilds a compact one.
// KMHG_COUNT_TABLE (tests): "adopt" adopts regardless of size, "rebuild" / "probe" never do.
bool adoptable(const kmhg_index* idx, const kmhg_index* B) {
  if (idx->U != 0 || B->u_upper) return false;   // a table sized by a key stream: rebuild
  if (const char* e = test_build_knob("KMHG_COUNT_TABLE")) return std::string(e) == "adopt";
  return B->slots() <= 6 * B->U;
}

void count_device(kmhg_index* idx, const uint8_t* d_seq, int64_t L, uint32_t source,
                  hipStream_t s) {
  ReleaseGroup rg(s);
  idx->stream = s;
  const int k = idx->k;
  if (L <= k) return;
  // the batch keeps its code words only to be eligible for bucket-id radix streams (<= 12 M
  // windows): a larger batch builds on key streams without them (no code block
  // allocated or written for a batch that is discarded after the merge); KMHG_COUNT_BID=0 (A/B)
  // builds every batch with key streams
  const char* cbe = test_build_knob("KMHG_COUNT_BID");
  const bool codes = !(cbe && cbe[0] == '0') && bid_streams_for(L - k + 1, read_build_knobs());
  std::unique_ptr<kmhg_index> B(build_device(d_seq, L, k, s, codes));
  Release rel{B.get(), s};
  finish_build(B.get());
  B->stream = s;
  if (!B->U) return;
  if (adoptable(idx, B.get()))
    adopt_first_batch(idx, B.get(), source, (uint64_t)idx->L, s);
  else
    merge_batch(idx, B.get(), source, (uint64_t)idx->L, s);
  idx->L += L;                     // the next batch's order keys start here
}

// Merge a batch index B (distinct keys with their counts in the slots) into the counts index,
// B's slots walked in slot order (empty slots skipped).  New keys get rows in that order;
// count.kmers rows get order keys base + first position - 1 (base = characters counted before
// the batch), so ensure_row_order can restore first-insertion order for a readout.
void merge_batch(kmhg_index* idx, kmhg_index* B, uint32_t source, uint64_t base, hipStream_t s) {
  ReleaseGroup rg(s);
  const int k = idx->k;
  const uint32_t S = idx->sources;
  const uint64_t Ub = B->U;
  const uint64_t U0 = idx->U;
  const bool ord = !idx->canonical;
  // KMHG_COUNT_TABLE (tests): "rebuild" / "probe" take the general merge even for the first batch
  const char* ct = test_build_knob("KMHG_COUNT_TABLE");
  if (adoptable(idx, B)) {         // first batch into an empty suffix hash
    adopt_first_batch(idx, B, source, base, s);
    return;
  }
  reserve_rows(idx, U0 + Ub, s);
  const uint64_t ni = B->slots();
  const uint32_t nt = tiles_for(ni);
  DBuf<uint32_t> rank(ni + 1, s);                 // flags -> ranks of the new keys; [ni] = total
  DBuf<uint64_t> status((size_t)nt + 1, s);
  HIPC(hipMemsetAsync(status.p, 0, ((size_t)nt + 1) * 8, s));
  LAUNCH("k_count_probe", s,
         launch_count_probe(nullptr, (uint32_t)ni, B->table.p, U0 ? idx->table.p : nullptr,
                            idx->geom, idx->slot_row.p, S, source, idx->positions.p, rank.p, s));
  LAUNCH("k_scan_u32", s, launch_scan_u32(rank.p, ni, status.p, rank.p + ni, s));
  LAUNCH("k_count_append", s,
         launch_count_append(nullptr, (uint32_t)ni, B->table.p, rank.p, rank.p + ni,
                             (uint32_t)U0, S, source, idx->ckeys.p, idx->positions.p,
                             ord ? B->positions.p : nullptr, ord ? idx->rord.p : nullptr, base,
                             s));
  uint32_t n_new = 0;
  HIPC(hipMemcpyAsync(&n_new, rank.p + ni, 4, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  const uint64_t U1 = U0 + n_new;
  // rebuild the table for U1 keys (aux of a source_n = 1 index carries the count itself, so
  // even a batch of known keys changes the slots): the partitioned build over the key list,
  // or global linear probing should a bucket overflow (never observed: a key list is distinct)
  idx->table.bind(s);
  idx->slot_row.bind(s);
  idx->row_slot.bind(s);
  // KMHG_COUNT_TABLE=probe: the fallback (tests)
  const bool probe_only = ct && std::string(ct) == "probe";
  std::unique_ptr<kmhg_index> K;
  bool ovf = true;
  if (!probe_only) {
    K.reset(build_device_v2(BuildRequest::key_stream(k, (int64_t)U1),
                            StreamPtrs{nullptr, idx->ckeys.p}, s));
    HIPC(hipEventSynchronize(K->rec.ev));
    ovf = K->rec.meta->overflow != 0;
    PinnedPool::get().give(K->rec, false);
    K->rec = PinnedRec{};
    K->pending = false;
  }
  Release relk{K ? K.get() : B, s};
  idx->row_slot.reset(U1);
  if (!ovf) {
    idx->geom = K->geom;
    idx->table.swap_with(K->table);
    idx->slot_row.reset(idx->slots());
    LAUNCH("k_count_fix", s, launch_count_fix(idx->table.p, idx->slots(), S, idx->positions.p,
                                              idx->slot_row.p, idx->row_slot.p, s));
  } else {
    idx->geom = Geom{1u, (uint32_t)table_capacity((int64_t)U1)};
    idx->table.reset(idx->slots());
    idx->slot_row.reset(idx->slots());
    LAUNCH("k_table_init", s, launch_table_init(idx->table.p, idx->slots(), s));
    LAUNCH("k_count_insert", s,
           launch_count_insert(idx->ckeys.p, (uint32_t)U1, idx->table.p, idx->geom, S,
                               idx->positions.p, idx->slot_row.p, idx->row_slot.p, s));
  }
  idx->U = U1;
  idx->N = U1 * S;
  idx->P = U1 * ((uint64_t)S * (S - 1) / 2);
  idx->max_n = U1 ? S : 0;
  idx->kmer_count += n_new;
  if (ord && n_new) idx->order_ready = false;
  idx->canon.ready = false;
}

// First-insertion order of a count.kmers index's rows (the order of their order keys, rord):
// C_place puts each row's index at F[rord], C_rows compacts F in order into rorder (rank ->
// row).  The rows stay where they are: the readout arrays (k_count_canon) and the export take
// them through rorder.  Run when a readout first asks for rows after a batch.
void ensure_row_order(kmhg_index* idx, hipStream_t s) {
  if (idx->order_ready || idx->canonical || !idx->U) return;
  ReleaseGroup rg(s);
  const uint64_t U = idx->U;
  const int64_t n = idx->L;                       // every order key is < the characters counted
  // F takes 4 B per character ever counted into the pointer (idx->L over all batches), which
  // grows with the input, not with the rows: beyond 8 characters per row (many sources or
  // batches of mostly known k-mers) the rows are ordered by a radix sort of their U order keys
  // instead, O(U) scratch (advisor, round 4).  KMHG_ROW_ORDER_SORT=1 / 0 forces the sort / F
  // (tests: both give the same order).
  const char* rse = test_build_knob("KMHG_ROW_ORDER_SORT");
  const bool by_sort = rse ? rse[0] == '1' : (uint64_t)n > 8 * U;
  if (by_sort) {
    int bits = 1;
    while (bits < 64 && (1ull << bits) < (uint64_t)n) ++bits;
    size_t tb = 0;
    HIPC(rows_sort_temp_bytes((uint32_t)U, bits, &tb));
    DBuf<uint64_t> keys_out(U, s);
    DBuf<uint32_t> rows_in(U, s);
    DBuf<uint8_t> temp(std::max<size_t>(tb, 16), s);
    idx->rorder.bind(s);
    idx->rorder.reset(U);
    hipError_t sort_err = hipSuccess;
    LAUNCH("k_rows_sort", s, sort_err = launch_rows_sort(idx->rord.p, (uint32_t)U, bits,
                                                         keys_out.p, rows_in.p, idx->rorder.p,
                                                         temp.p, tb, s));
    HIPC(sort_err);                 // rorder is not valid unless the sort ran
    idx->order_ready = true;
    return;
  }
  DBuf<uint32_t> F((size_t)n, s);
  HIPC(hipMemsetAsync(F.p, 0xFF, (size_t)n * 4, s));
  LAUNCH("k_rows_place", s, launch_rows_place(idx->rord.p, (uint32_t)U, F.p, s));
  const uint64_t nt = ((uint64_t)n + TILE - 1) / TILE;
  DBuf<uint64_t> status(nt + 1, s);               // look-back words + the tile ticket
  HIPC(hipMemsetAsync(status.p, 0, (nt + 1) * 8, s));
  idx->rorder.bind(s);
  idx->rorder.reset(U);
  LAUNCH("k_rows_order", s,
         launch_rows_order(F.p, n, status.p, reinterpret_cast<uint32_t*>(status.p + nt),
                           idx->rorder.p, s));
  idx->order_ready = true;
}

// rorder of a counts index, or nullptr when its rows are already in order (a suffix hash)
const uint32_t* row_order_of(const kmhg_index* idx) {
  return idx->canonical ? nullptr : idx->rorder.p;
}

// ---------------------------------------------------------------------------- read counting
// count.kmers.fq.sh.rp / seq.kmer.depth.sh / kmer.spec.sh.n (kmhg_sh.hip).  The suffix_hash_n
// of the reference is a counts index of canonical k-mers (canonical = true, sources = counts_n).
// The host side -- a call's parameters (ReadCall), the packed host reads and their reader, the
// split into device batches, the quality table's formula -- is kmhg_reads.h (no HIP); here are
// the device batches, the uploads and the launch sequences.

// q_to_ll's table (qll_host, kmhg_reads.h), uploaded once per device.
const double* qll_device(hipStream_t s) {
  static std::mutex mu;
  static std::map<int, double*> tables;
  int dev = 0;
  HIPC(hipGetDevice(&dev));
  std::lock_guard<std::mutex> g(mu);
  auto it = tables.find(dev);
  if (it != tables.end()) return it->second;
  double h[256];
  for (int q = 0; q < 256; ++q) h[q] = qll_host(q);
  double* d = static_cast<double*>(DevicePool::get().alloc(sizeof h));
  HIPC(hipMemcpyAsync(d, h, sizeof h, hipMemcpyHostToDevice, s));
  HIPC(hipStreamSynchronize(s));
  tables[dev] = d;
  return d;
}

// The count-only partitioned build of a key stream at `spread` (0: from its HLL estimate),
// waited for.  `overflow`: a bucket's LDS sub-table filled up -- the table is unusable and the
// caller retries at spread 1 (the index still reports the spread and estimate it tried).
// `keys` is a padded stream (EMPTY_KEY entries skipped, k <= 31).
std::unique_ptr<kmhg_index> count_only_build(const uint64_t* keys, uint32_t total, int k,
                                             int spread, hipStream_t s, bool& overflow) {
  std::unique_ptr<kmhg_index> B(build_device_v2(
      BuildRequest::count_keys(k, (int64_t)total, spread), StreamPtrs{nullptr, keys}, s));
  HIPC(hipEventSynchronize(B->rec.ev));
  const BuildMeta hm = *B->rec.meta;
  PinnedPool::get().give(B->rec, false);
  B->rec = PinnedRec{};
  B->pending = false;
  B->stream = s;
  if (!B->co_spread) B->co_spread = spread;
  overflow = hm.overflow != 0;
  B->U = overflow ? 0 : hm.n_kmers;
  return B;
}

kmhg_index* new_sh_index(int k, int counts_n, hipStream_t s) {
  auto idx = std::make_unique<kmhg_index>();
  HIPC(hipGetDevice(&idx->device));
  idx->k = k;
  idx->sources = (uint32_t)counts_n;
  idx->canonical = true;
  idx->stream = s;
  idx->geom = Geom{1u, 8u};                      // an empty table: lookups before any count
  idx->table.reset(idx->slots());
  LAUNCH("k_table_init", s, launch_table_init(idx->table.p, idx->slots(), s));
  return idx.release();
}

// One batch of packed reads (device-resident) merged into the suffix hash: per-read upper
// bounds (R_ub) -> scan -> R_kmers emit, padded with EMPTY_KEY up to each read's bound ->
// partitioned build of the key stream, padding skipped (occurrence counts per distinct key) ->
// merge over the batch table's slots.  The padding (quality- or N-rejected windows) costs its
// 8 B per window in the build's first pass; the exact count pass it replaces re-walked every
// read and cost a second host round trip (reads leg: see DESIGN.md).
void sh_count_reads_device(kmhg_index* idx, const uint8_t* d_seq, const uint8_t* d_qual,
                           const int64_t* d_off, const uint8_t* d_hasq, uint32_t n_reads,
                           const ReadWalk& walk, hipStream_t s) {
  ReleaseGroup rg(s);
  idx->stream = s;
  if (!n_reads) return;
  const int k = idx->k;
  const uint32_t source = walk.source;
  const double* qll = walk.sh1 ? nullptr : qll_device(s);
  DBuf<uint32_t> cnt((size_t)n_reads + 1, s);
  DBuf<int64_t> eend;                              // sh1: each record's end (its first NUL)
  const uint32_t nt = tiles_for(n_reads);
  // scan look-back + ticket, then the span and (sh1) the number of records without qualities
  DBuf<uint64_t> status((size_t)nt + 2, s);
  HIPC(hipMemsetAsync(status.p, 0, ((size_t)nt + 2) * 8, s));
  uint32_t* d_span = reinterpret_cast<uint32_t*>(status.p + nt + 1);
  LAUNCH("k_rk_span", s, launch_rk_span(d_off, n_reads, d_span, s));
  if (walk.sh1) {
    eend.reset(n_reads);
    eend.bind(s);
    LAUNCH("k_sh1_ub", s, launch_sh1_ub(d_off, d_hasq, n_reads, k, cnt.p, eend.p, d_span + 1, s));
  } else {
    LAUNCH("k_read_ub", s, launch_read_ub(d_off, n_reads, k, cnt.p, s));
  }
  LAUNCH("k_scan_u32", s, launch_scan_u32(cnt.p, n_reads, status.p, cnt.p + n_reads, s));
  // one round trip for the staging span and the stream length (pinned: the GiveBack returns it)
  PinnedRec hr = PinnedPool::get().take();
  GiveBack hr_back{hr, s};
  HIPC(hipMemcpyAsync(&hr.meta->n_pairs, d_span, 8, hipMemcpyDeviceToHost, s));
  HIPC(hipMemcpyAsync(&hr.meta->max_count, cnt.p + n_reads, 4, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  const uint64_t span_noq = __atomic_load_n(&hr.meta->n_pairs, __ATOMIC_ACQUIRE);
  const uint32_t span = (uint32_t)span_noq, n_noq = (uint32_t)(span_noq >> 32);
  const uint32_t total = __atomic_load_n(&hr.meta->max_count, __ATOMIC_ACQUIRE);
  const char* rkc = test_build_knob("KMHG_RK_CAP");   // A/B knob: LDS bytes per stream (16: global)
  const uint32_t cap = rkc ? (((uint32_t)std::atoi(rkc) + 15) & ~15u) : read_kmers_cap_span(span);
  if (!total) return;
  DBuf<uint64_t> keys(total, s);
  if (!walk.sh1) {
    LAUNCH("k_read_kmers_emit", s,
           launch_read_kmers(d_seq, d_qual, d_off, d_hasq, n_reads, k, walk.min_ll, qll, cap,
                             cnt.p, keys.p, s));
  } else {
    // routed by record: qualities -> the lane-per-read walk, none -> the position-parallel
    // kernel (a chromosome-length FASTA record would otherwise be one lane's serial walk)
    if (n_noq < n_reads)
      LAUNCH("k_read_kmers_sh1", s,
             launch_read_kmers_sh1(d_seq, d_qual, d_off, d_hasq, n_reads, k, walk.mq, cap, cnt.p,
                                   keys.p, s));
    if (n_noq) {
      int64_t ends[2] = {0, 0};
      HIPC(hipMemcpyAsync(&ends[0], d_off, 8, hipMemcpyDeviceToHost, s));
      HIPC(hipMemcpyAsync(&ends[1], d_off + n_reads, 8, hipMemcpyDeviceToHost, s));
      HIPC(hipStreamSynchronize(s));
      const int64_t span16 = ends[1] - (ends[0] & ~(int64_t)15);
      if (span16 > 0) {
        LAUNCH("k_sh1_nul", s, launch_sh1_nul(d_seq, d_off, n_reads, span16, eend.p, s));
        LAUNCH("k_fa_kmers", s,
               launch_fa_kmers(d_seq, d_off, eend.p, d_hasq, n_reads, k, span16, cnt.p, keys.p,
                               s));
      }
    }
  }
  // The count-only build gives each group bucket `spread` x V2_BW_WG stream entries, so that the
  // batch's distinct keys -- not its key stream -- fill the LDS sub-tables (bench, 3.7x
  // coverage: spread 1/2/3/4 -> 22.6/26.8/28.5/27.6 Gbp/s).  The spread comes from THIS
  // batch's HLL estimate of its distinct keys (build_device_v2, co_spread = 0).
  // KMHG_CO_GLOBAL=1 (tests): straight to the global fallback below
  const bool force_global = test_build_knob("KMHG_CO_GLOBAL") != nullptr;
  std::unique_ptr<kmhg_index> B;
  bool ovf = true;
  int path = 1;
  double est = 0.0;
  int spread = 0;
  if (!force_global) {
    B = count_only_build(keys.p, total, k, 0, s, ovf);
    est = B->co_est;
    spread = B->co_spread;
    if (ovf && spread > 1) {                     // a sub-table overflowed: spread 1 (mean 1024)
      path = 2;
      B->bind_all(s);
      B = count_only_build(keys.p, total, k, 1, s, ovf);
    }
  }
  if (ovf) {                                     // still overflowing: global find-or-insert
    path = 3;
    if (B) B->bind_all(s);
    B = std::make_unique<kmhg_index>();
    HIPC(hipGetDevice(&B->device));
    B->k = k;
    B->stream = s;
    B->geom = Geom{1u, (uint32_t)table_capacity((int64_t)total)};
    B->table.reset(B->slots());
    LAUNCH("k_table_init", s, launch_table_init(B->table.p, B->slots(), s));
    LAUNCH("k_key_count_insert", s,
           launch_key_count_insert(keys.p, total, B->table.p, B->geom, s));
    B->U = total;                                // an upper bound (row capacity only)
    B->u_upper = true;                           // sized by the stream: never adopted
  }
  Release rel{B.get(), s};
  idx->co_est = est;
  idx->co_spread = spread;
  idx->co_path = path;
  if (B->U == 0) return;                         // every window of the batch rejected
  merge_batch(idx, B.get(), source, 0, s);
}

// The split point of sh_count_reads_host.  KMHG_SH_SPAN (test build) lowers it, so that the
// sub-range calls -- offsets that do not start at 0 -- run at test sizes.
static uint64_t sh_host_span_max() {
  if (const char* e = test_build_knob("KMHG_SH_SPAN")) {
    const uint64_t v = std::strtoull(e, nullptr, 10);
    if (v > 0 && v < SH_SPAN_MAX) return v;
  }
  return SH_SPAN_MAX;
}

// Packed host reads uploaded once and counted in read_batches' device batches (the device pass
// sizes its key stream by per-read window bounds summed in u32); idx->L gains their bases.
void sh_count_reads_host(kmhg_index* idx, const ReadsHost& r, const ReadWalk& walk,
                         hipStream_t s) {
  const size_t n = r.n();
  std::vector<std::pair<size_t, size_t>> batches;
  const Refusal bad = read_batches(r.off.data(), n, sh_host_span_max(), batches);
  if (bad.err) fail(bad.err, bad.msg);
  if (!n) return;
  const size_t nb = r.seq.size();
  DBuf<uint8_t> dseq(nb + 16, s), dqual(nb + 16, s), dhq(n, s);
  DBuf<int64_t> doff(n + 1, s);
  HIPC(hipMemcpyAsync(dseq.p, r.seq.data(), nb, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(dqual.p, r.qual.data(), nb, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(dhq.p, r.hasq.data(), n, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(doff.p, r.off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  for (const auto& b : batches)
    sh_count_reads_device(idx, dseq.p, dqual.p, doff.p + b.first, dhq.p + b.first,
                          (uint32_t)(b.second - b.first), walk, s);
  HIPC(hipStreamSynchronize(s));                 // the host arrays are reused
  idx->L += (int64_t)nb;
}

void sh_depth_device(kmhg_index* idx, const uint8_t* d_seq, int64_t L, int k, int32_t* d_out,
                     hipStream_t s) {
  ReleaseGroup rg(s);
  idx->stream = s;
  const uint32_t S = idx->sources;
  if (L > 0)
    HIPC(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_out), (int)INT_MIN,
                           (size_t)L * S, s));
  if (L <= 0) return;
  const uint32_t nt = depth_tiles(L);
  DBuf<uint32_t> tcnt((size_t)nt + 1, s);
  const uint32_t ntt = tiles_for(nt);
  DBuf<uint64_t> status((size_t)ntt + 1, s);
  HIPC(hipMemsetAsync(status.p, 0, ((size_t)ntt + 1) * 8, s));
  LAUNCH("k_depth_seg_count", s, launch_depth_seg_count(d_seq, L, tcnt.p, s));
  LAUNCH("k_scan_u32", s, launch_scan_u32(tcnt.p, nt, status.p, tcnt.p + nt, s));
  uint32_t M = 0;
  HIPC(hipMemcpyAsync(&M, tcnt.p + nt, 4, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  DBuf<uint32_t> seg((size_t)2 * M + 2, s);
  DBuf<uint8_t> stale((size_t)M + 1, s);
  uint32_t* sstart = seg.p;
  uint32_t* send = seg.p + M + 1;
  if (M) LAUNCH("k_depth_seg_emit", s, launch_depth_seg_emit(d_seq, L, tcnt.p, sstart, send, s));
  LAUNCH("k_depth_modes", s,
         launch_depth_modes(d_seq, L, k, sstart, send, tcnt.p + nt, stale.p, idx->table.p,
                            idx->geom, S, idx->positions.p, d_out, s));
  if (M)
    LAUNCH("k_depth_probe", s,
           launch_depth_probe(d_seq, L, k, sstart, send, tcnt.p + nt, stale.p, idx->table.p,
                              idx->geom, S, idx->positions.p, d_out, s));
}

void check_sh(const kmhg_index* idx) {
  if (!idx || !idx->canonical || idx->single)
    fail(KMHG_EINVAL, "unable to obtain suffix_hash_n from external pointer");
}

// ---------------------------------------------------------------------------- readout
uint32_t side_bucket_of(uint32_t nb);
// The slots a readout walks: a part's side slot is written only by the part that owns its
// bucket (kmhg_part_info's info[8]); elsewhere it is not part of the table.
uint64_t read_slots(const kmhg_index* idx) {
  if (!idx->is_part) return idx->slots();
  const Geom& G = idx->geom;
  const uint32_t side_b = side_bucket_of(G.nbh);
  const bool owns = G.nb && side_b >= G.b0 && side_b < G.b0 + G.nb;
  return (uint64_t)G.nb * G.capb + (owns ? 1 : 0);
}

void prepare_canon(kmhg_index* idx, hipStream_t s) {
  ReleaseGroup rg(s);
  idx->stream = s;
  Canon& c = idx->canon;
  if (c.ready) return;
  if (idx->sources) {            // counts index: rows in first-insertion order (ensure_row_order)
    ensure_row_order(idx, s);
    const uint32_t U = (uint32_t)idx->U, S = idx->sources;
    c.perm.reset(U);
    c.canon_off.reset(U + 1);
    c.pkeys.reset(S >= 2 ? U : 1);
    c.pair_off.reset(S >= 2 ? U : 1);
    c.rinfo.reset(U);
    LAUNCH("k_count_canon", s, launch_count_canon(row_order_of(idx), idx->row_slot.p,
                                                  idx->positions.p, U, S, c.perm.p,
                                                  c.canon_off.p, c.pkeys.p, c.pair_off.p,
                                                  c.rinfo.p, s));
    c.n_multi = S >= 2 ? U : 0;
    c.ready = true;
    return;
  }
  const int64_t L = idx->L;
  const uint32_t U = (uint32_t)idx->U;
  DBuf<uint2> F(L, s);
  HIPC(hipMemsetAsync(F.p, 0xFF, (size_t)L * 8, s));
  if (U) LAUNCH("k_read_first", s, launch_read_first(idx->table.p, read_slots(idx),
                                                     idx->positions.p, F.p, s));
  const uint32_t nt = tiles_for(L);
  const size_t scratch_bytes = (size_t)nt * 24 + 64 + sizeof(ReadMeta);
  DBuf<uint8_t> scratch(scratch_bytes, s);
  HIPC(hipMemsetAsync(scratch.p, 0, scratch_bytes, s));
  uint64_t* st_a = reinterpret_cast<uint64_t*>(scratch.p);
  uint64_t* st_b = st_a + nt;
  uint64_t* st_c = st_b + nt;
  uint32_t* ticket = reinterpret_cast<uint32_t*>(scratch.p + (size_t)nt * 24);
  ReadMeta* rm = reinterpret_cast<ReadMeta*>(scratch.p + (size_t)nt * 24 + 64);
  c.perm.reset(U);
  c.canon_off.reset(U + 1);
  c.rinfo.reset(U);
  // keys with >= 2 positions: at most N/2
  c.pkeys.reset(idx->N / 2 + 1);
  c.pair_off.reset(idx->N / 2 + 1);
  LAUNCH("k_read_order", s,
         launch_read_order(F.p, L, idx->table.p, st_a, st_b, st_c, ticket, c.perm.p,
                           c.canon_off.p, c.pkeys.p, c.pair_off.p, c.rinfo.p, rm, s));
  ReadMeta h;
  HIPC(hipMemcpyAsync(&h, rm, sizeof(h), hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  if (h.n_keys != idx->U || h.n_rows != idx->N || h.n_pairs != idx->P)
    fail(KMHG_EDEVICE, "readout order inconsistent with the index (internal error)");
  c.n_multi = h.n_multi;
  c.ready = true;
}

// Readout arrays for idx->row_order.  The first-occurrence arrays are built on the GPU
// (prepare_canon); the khash order relabels them: the keys go to the host once, the bucket
// order is replayed there (inherently sequential, ~0.1 us per key), and the permuted arrays
// come back.  The readout kernels then run unchanged.
void prepare_readout(kmhg_index* idx, hipStream_t s) {
  ReleaseGroup rg(s);
  finish_build(idx);
  Canon& c = idx->canon;
  if (c.ready && c.order == idx->row_order) return;
  if (c.ready && c.order != KMHG_ORDER_FIRST) c.ready = false;   // rebuild from first order
  prepare_canon(idx, s);
  c.order = KMHG_ORDER_FIRST;
  if (idx->row_order == KMHG_ORDER_FIRST) return;
  const uint32_t U = (uint32_t)idx->U;
  std::vector<uint64_t> keys(U);
  std::vector<uint32_t> perm(U);
  std::vector<uint2> info(U);
  if (U) {
    DBuf<uint64_t> dk(U, s);
    LAUNCH("k_gather_keys", s, launch_gather_keys(c.perm.p, U, idx->table.p, dk.p, s));
    HIPC(hipMemcpyAsync(keys.data(), dk.p, (size_t)U * 8, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(info.data(), c.rinfo.p, (size_t)U * 8, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(perm.data(), c.perm.p, (size_t)U * 4, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
  }
  const std::vector<uint32_t> order = khash_bucket_order(keys);
  if (order.size() != U) fail(KMHG_EDEVICE, "khash order replay lost keys (internal error)");
  std::vector<uint32_t> perm_k(U), off_k(U + 1), pkeys;
  std::vector<uint2> info_k(U);
  std::vector<uint64_t> pair_off;
  uint64_t rows = 0, pairs = 0;
  for (uint32_t r = 0; r < U; ++r) {
    const uint32_t id = order[r];
    const uint64_t n = (uint64_t)info[id].x;
    perm_k[r] = perm[id];
    info_k[r] = info[id];
    off_k[r] = (uint32_t)rows;
    rows += n;
    if (n >= 2) {
      pkeys.push_back(r);
      pair_off.push_back(pairs);
      pairs += n * (n - 1) / 2;
    }
  }
  off_k[U] = (uint32_t)rows;
  if (rows != idx->N || pairs != idx->P || pkeys.size() != c.n_multi)
    fail(KMHG_EDEVICE, "khash readout order inconsistent with the index (internal error)");
  if (U) {
    HIPC(hipMemcpyAsync(c.perm.p, perm_k.data(), (size_t)U * 4, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(c.rinfo.p, info_k.data(), (size_t)U * 8, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(c.canon_off.p, off_k.data(), (size_t)(U + 1) * 4, hipMemcpyHostToDevice, s));
  }
  if (!pkeys.empty()) {
    HIPC(hipMemcpyAsync(c.pkeys.p, pkeys.data(), pkeys.size() * 4, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(c.pair_off.p, pair_off.data(), pair_off.size() * 8,
                        hipMemcpyHostToDevice, s));
  }
  HIPC(hipStreamSynchronize(s));   // host vectors die here
  c.order = KMHG_ORDER_KHASH;
}

void positions_sizes(kmhg_index* idx, uint32_t opt, int64_t* nk, int64_t* np, int64_t* npp,
                     int64_t* nc) {
  if (idx->canonical) fail(KMHG_EINVAL, "External pointer has incorrect tag");
  if (nk) *nk = (opt & KMHG_OPT_KMER) ? (int64_t)idx->U : 0;
  if (np) *np = (opt & KMHG_OPT_POS) ? (int64_t)idx->N : 0;
  if (npp) *npp = (opt & KMHG_OPT_PAIRS) ? (int64_t)idx->P : 0;
  if (nc) *nc = (opt & KMHG_OPT_COUNT) ? (int64_t)idx->U : 0;
}

void positions_device(kmhg_index* idx, uint32_t opt, char* kmers, int32_t* pos, int32_t* pairs,
                      int32_t* counts, hipStream_t s) {
  ReleaseGroup rg(s);
  if (idx->canonical) fail(KMHG_EINVAL, "External pointer has incorrect tag");
  if (idx->is_part) fail(KMHG_EINVAL, "a part index must be assembled before it is read");
  prepare_readout(idx, s);
  Canon& c = idx->canon;
  const uint32_t U = (uint32_t)idx->U;
  if ((opt & (KMHG_OPT_KMER | KMHG_OPT_COUNT)) && U)
    LAUNCH("k_read_keys", s,
           launch_read_keys(c.perm.p, c.rinfo.p, U, idx->table.p, idx->k,
                            (opt & KMHG_OPT_COUNT) ? counts : nullptr,
                            (opt & KMHG_OPT_KMER) ? kmers : nullptr, s));
  if ((opt & KMHG_OPT_POS) && idx->N) {
    DBuf<uint32_t> tile_key((size_t)read_pos_tiles(idx->N) + 1, s);
    LAUNCH("k_read_pos", s,
           launch_read_pos(c.rinfo.p, c.canon_off.p, U, idx->N, idx->positions.p, tile_key.p,
                           reinterpret_cast<int2*>(pos), s));
  }
  if ((opt & KMHG_OPT_PAIRS) && idx->P) {
    DBuf<uint32_t> tile_key((size_t)read_pairs_tiles(idx->P) + 1, s);
    LAUNCH("k_read_pairs", s,
           launch_read_pairs(c.pkeys.p, c.pair_off.p, (uint32_t)c.n_multi, idx->P, c.rinfo.p,
                             idx->positions.p, tile_key.p, pairs, s));
  }
}

// ------------------------------------------------------------------ kmer.pos over resident parts
// kmer.pos (src/kmer_hash.c:1054-1147) of an index that stays split in its owner-computes parts
// (src/kmer_reader.c:28-39): kmhg_parts_read.h.  A part is read in its own first-occurrence
// order (prepare_canon over its slots), which is ascending global label.
kmhg_index* check_part_read(kmhg_index* idx) {
  if (!idx) fail(KMHG_EINVAL, "null index");
  if (!idx->is_part) fail(KMHG_EINVAL, "not a part index");
  return idx;
}

void part_first_mask(kmhg_index* idx, uint32_t* mask, hipStream_t s) {
  ReleaseGroup rg(s);
  finish_build(idx);
  idx->stream = s;
  HIPC(hipMemsetAsync(mask, 0, mask_words(idx->L) * 4, s));
  if (idx->U)                    // (a part that owns no bucket has no table to walk)
    LAUNCH("k_part_mask", s,
           launch_part_mask(idx->table.p, read_slots(idx), idx->positions.p, idx->L, mask, s));
}

void part_positions_device(kmhg_index* idx, const uint32_t* mask, uint32_t opt, int32_t* labels,
                           char* kmers, int32_t* pos, int32_t* pairs, int32_t* counts,
                           hipStream_t s) {
  ReleaseGroup rg(s);
  finish_build(idx);
  if (idx->row_order != KMHG_ORDER_FIRST)
    fail(KMHG_EINVAL, "kmer.pos over parts is in first-occurrence order only (the khash order "
                      "needs every key on one host: assemble the parts)");
  const uint32_t U = (uint32_t)idx->U;
  if (!U) return;
  if (!mask || !labels) fail(KMHG_EINVAL, "null argument");
  if (((opt & KMHG_OPT_KMER) && !kmers) || ((opt & KMHG_OPT_COUNT) && !counts) ||
      ((opt & KMHG_OPT_POS) && idx->N && !pos) || ((opt & KMHG_OPT_PAIRS) && idx->P && !pairs))
    fail(KMHG_EINVAL, "null output for a requested opt bit");
  prepare_canon(idx, s);
  Canon& c = idx->canon;
  const uint64_t W = mask_words(idx->L);
  const uint32_t nt = tiles_for(W);
  DBuf<uint32_t> wprefix(W, s);
  DBuf<uint64_t> status((size_t)nt + 1, s);        // look-back words, then the ticket
  HIPC(hipMemsetAsync(status.p, 0, ((size_t)nt + 1) * 8, s));
  LAUNCH("k_mask_prefix", s,
         launch_mask_prefix(mask, W, status.p, reinterpret_cast<uint32_t*>(status.p + nt),
                            wprefix.p, s));
  LAUNCH("k_part_labels", s,
         launch_part_labels(c.rinfo.p, U, idx->positions.p, mask, wprefix.p, W, labels, s));
  if (opt & (KMHG_OPT_KMER | KMHG_OPT_COUNT))
    LAUNCH("k_read_keys", s,
           launch_read_keys(c.perm.p, c.rinfo.p, U, idx->table.p, idx->k,
                            (opt & KMHG_OPT_COUNT) ? counts : nullptr,
                            (opt & KMHG_OPT_KMER) ? kmers : nullptr, s));
  if ((opt & KMHG_OPT_POS) && idx->N) {
    DBuf<uint32_t> tile_key((size_t)read_pos_tiles(idx->N) + 1, s);
    LAUNCH("k_read_pos_labels", s,
           launch_read_pos_labels(c.rinfo.p, c.canon_off.p, U, idx->N, idx->positions.p,
                                  tile_key.p, labels, reinterpret_cast<int2*>(pos), s));
  }
  if ((opt & KMHG_OPT_PAIRS) && idx->P) {
    DBuf<uint32_t> tile_key((size_t)read_pairs_tiles(idx->P) + 1, s);
    LAUNCH("k_read_pairs_labels", s,
           launch_read_pairs_labels(c.pkeys.p, c.pair_off.p, (uint32_t)c.n_multi, idx->P,
                                    c.rinfo.p, idx->positions.p, tile_key.p, labels, pairs, s));
  }
  HIPC(hipGetLastError());
}

// The root's merge.  Per-key row runs keep their order inside a part, so a run only needs the
// difference between where it starts in the whole result (the scan of the merged counts) and
// where it starts in its part (the scan of the part's counts): delta, indexed by label.
void merge_part_positions(int n_parts, uint32_t opt, int k, const int64_t* nk, const int64_t* np,
                          const int64_t* npp, const int32_t* const* labels,
                          const int32_t* const* counts, const char* const* kmers,
                          const int32_t* const* pos, const int32_t* const* pairs, char* o_kmers,
                          int32_t* o_pos, int32_t* o_pairs, int32_t* o_counts, hipStream_t s) {
  ReleaseGroup rg(s);
  const bool want_pos = opt & KMHG_OPT_POS, want_pairs = opt & KMHG_OPT_PAIRS;
  const bool need_counts = want_pos || want_pairs || (opt & KMHG_OPT_COUNT);
  uint64_t Ut = 0, Nt = 0, Pt = 0, Umax = 0;
  for (int r = 0; r < n_parts; ++r) {
    if (nk[r] < 0 || (want_pos && np[r] < 0) || (want_pairs && npp[r] < 0))
      fail(KMHG_EINVAL, "bad merge arguments");
    Ut += (uint64_t)nk[r];
    Umax = std::max<uint64_t>(Umax, (uint64_t)nk[r]);
    if (want_pos) Nt += (uint64_t)np[r];
    if (want_pairs) Pt += (uint64_t)npp[r];
    if (nk[r] && (!labels[r] || (need_counts && !counts[r]) ||
                  ((opt & KMHG_OPT_KMER) && !kmers[r]) || (want_pos && np[r] && !pos[r]) ||
                  (want_pairs && npp[r] && !pairs[r])))
      fail(KMHG_EINVAL, "null argument");
  }
  if (Ut > (uint64_t)INT32_MAX || Nt > (uint64_t)INT32_MAX || Pt > (uint64_t)INT32_MAX)
    fail(KMHG_EOVERFLOW, "result has more than 2^31-1 rows");
  if (!Ut) return;
  if (((opt & KMHG_OPT_KMER) && !o_kmers) || ((opt & KMHG_OPT_COUNT) && !o_counts) ||
      (want_pos && Nt && !o_pos) || (want_pairs && Pt && !o_pairs))
    fail(KMHG_EINVAL, "null output for a requested opt bit");
  const uint32_t U = (uint32_t)Ut;
  DBuf<int32_t> gc_own;
  int32_t* gcount = nullptr;
  if (need_counts) {
    if (opt & KMHG_OPT_COUNT) gcount = o_counts;
    else { gc_own.reset(U); gc_own.bind(s); gcount = gc_own.p; }
  }
  for (int r = 0; r < n_parts; ++r)
    if (nk[r])
      LAUNCH("k_merge_keys", s,
             launch_merge_keys(labels[r], need_counts ? counts[r] : nullptr,
                               (opt & KMHG_OPT_KMER) ? kmers[r] : nullptr, (uint32_t)nk[r], k, U,
                               gcount, (opt & KMHG_OPT_KMER) ? o_kmers : nullptr, s));
  if ((want_pos && Nt) || (want_pairs && Pt)) {
    DBuf<uint64_t> goff(U, s), loff(Umax, s), scr(scan_u64_scratch(U) + 1, s), total(2, s);
    DBuf<int64_t> delta(U, s);
    for (int pass = 0; pass < 2; ++pass) {           // pos rows, then pair rows
      const bool pr = pass == 1;
      const uint64_t n_out = pr ? Pt : Nt;
      if (!(pr ? want_pairs : want_pos) || !n_out) continue;
      LAUNCH("k_rows_per_key", s, launch_rows_per_key(gcount, U, pr, goff.p, s));
      LAUNCH("k_scan_u64", s, launch_scan_u64(goff.p, U, total.p, scr.p, s));
      for (int r = 0; r < n_parts; ++r) {
        const uint64_t nr = (uint64_t)(pr ? npp[r] : np[r]);
        if (!nk[r] || !nr) continue;
        const uint32_t Up = (uint32_t)nk[r];
        LAUNCH("k_rows_per_key", s, launch_rows_per_key(counts[r], Up, pr, loff.p, s));
        LAUNCH("k_scan_u64", s, launch_scan_u64(loff.p, Up, total.p + 1, scr.p, s));
        LAUNCH("k_merge_delta", s,
               launch_merge_delta(labels[r], loff.p, goff.p, Up, U, delta.p, s));
        LAUNCH("k_merge_rows", s,
               launch_merge_rows(pr ? pairs[r] : pos[r], nr, pr ? 3 : 2, delta.p, U, n_out,
                                 pr ? o_pairs : o_pos, s));
      }
    }
  }
  HIPC(hipGetLastError());
}

// ------------------------------------------------------------------ multi-device seq.kmer.pos
// KMHG_DEVICES=d0,d1,... (SURVEY.md §5 "Config / flags"): the host-pointer seq.kmer.pos of the
// R API (.Call("sequence_kmer_positions"), src/kmer_hash.c:1151-1172) is split over these
// devices in one process, with the R signatures unchanged.  The index is replicated once per
// device by peer copies over xGMI (the image: table + positions + code block), the query's
// windows are cut into contiguous ranges (the multi-GPU shard unit of
// kmhg_query_run_device_range), each device receives only its range's slice of the host
// sequence (plus the neighbour chars the window rule reads) and queries it on its own host
// thread, and the rows stay in each device's HBM until kmhg_query_fill copies every part
// straight into the caller's buffer at its prefix offset.  Concatenation in range order is the
// unsharded row order.
void free_index(kmhg_index* idx);
void free_query(kmhg_query* q);

// the bucket holding the side slot's key ~0 (bucket_of(mix64(~0), nb), kmhg_device.h) on the host
uint32_t side_bucket_of(uint32_t nb) {
  return (uint32_t)(((unsigned __int128)mix64(EMPTY_KEY) * nb) >> 64);
}

std::vector<int> query_devices() {
  std::vector<int> out;
  const char* e = std::getenv("KMHG_DEVICES");
  if (!e || !*e) return out;
  int n = 0;
  HIPC(hipGetDeviceCount(&n));
  const DeviceList bad = parse_device_list(e, n, out);
  if (bad.code != KMHG_OK) fail(bad.code, bad.text);
  return out;
}

// A copy of `home` on device `dev`, by peer copies (hipMemcpyPeerAsync: xGMI between MI355X
// GPUs; a same-device copy when dev is home's own device).  Its diagonal-path bits and slot
// tags are derived by its own first query, as for an imported image.
kmhg_index* make_replica(kmhg_index* home, int dev) {
  auto r = std::make_unique<kmhg_index>();
  r->device = dev;
  r->k = home->k; r->L = home->L; r->geom = home->geom;
  r->U = home->U; r->N = home->N; r->P = home->P; r->max_n = home->max_n;
  r->kmer_count = home->kmer_count;
  r->row_order = home->row_order;
  DeviceGuard g(dev);
  hipStream_t s = lib_stream();
  r->stream = s;
  r->table.reset(home->slots());
  HIPC(hipMemcpyPeerAsync(r->table.p, dev, home->table.p, home->device,
                          home->slots() * sizeof(Slot), s));
  if (home->N) {
    r->positions.reset(home->N);
    HIPC(hipMemcpyPeerAsync(r->positions.p, dev, home->positions.p, home->device, home->N * 4,
                            s));
  }
  if (home->dcodes.p) {
    const uint64_t w = diag_block_words(home->L - home->k + 1);
    r->dcodes.reset(w);
    HIPC(hipMemcpyPeerAsync(r->dcodes.p, dev, home->dcodes.p, home->device, w * 8, s));
  }
  HIPC(hipStreamSynchronize(s));
  return r.release();
}

// The index's copy on device `dev` (one per device, shared by every query part that runs
// there; made on first use, freed with the index).
kmhg_index* replica_on(kmhg_index* home, int dev) {
  {
    std::lock_guard<std::mutex> lk(home->rep_mu);
    auto it = home->replicas.find(dev);
    if (it != home->replicas.end()) return it->second;
  }
  kmhg_index* r = make_replica(home, dev);          // outside the lock: devices copy in parallel
  std::lock_guard<std::mutex> lk(home->rep_mu);
  auto& slot = home->replicas[dev];
  if (slot) {                                       // another thread made it meanwhile
    free_index(r);
    return slot;
  }
  slot = r;
  return r;
}

kmhg_query* query_multi_device(kmhg_index* idx, const char* seq, const QueryCall& whole,
                               const std::vector<int>& devs) {
  {
    DeviceGuard g(idx->device);
    finish_build(idx);
    if (idx->canonical) fail(KMHG_EINVAL, "External pointer has incorrect tag");
  }
  // (the slices shard_chars cuts carry no halo of w - 1 windows for the selection rule)
  if (idx->sampling > 1) fail(KMHG_EINVAL, "a sampled index is queried on its own device");
  const int G = (int)devs.size();
  const int64_t L = whole.L;
  auto q = std::make_unique<kmhg_query>();
  q->device = idx->device;
  q->parts.assign(G, nullptr);                       // freed with q, also on the error path
  const bool poison = test_build_knob("KMHG_SLICE_POISON") != nullptr;   // tests: garbage outside
  // tests: parts after the first on the index's own device use a same-device replica, so the
  // copy path runs on a one-GPU box too
  const bool test_replica = test_build_knob("KMHG_TEST_REPLICA") != nullptr;
  // one host thread per distinct device; the parts of one device run in order on its thread
  // (they share that device's stream and index copy)
  const Error bad = for_parts(devs, [&](int i) {
    const Span64 w = shard_windows(whole.w1, i, G);
    const bool home = devs[i] == idx->device && !(test_replica && i > 0);
    kmhg_index* use = home ? idx : replica_on(idx, devs[i]);
    DeviceGuard g(devs[i]);
    hipStream_t s = lib_stream();
    // a full-length buffer holding only the chars the part's windows may read (shard_chars)
    const Span64 ch = shard_chars(L, whole.k, w.begin, w.end);
    DBuf<uint8_t> d((size_t)L + 16, s);
    if (poison) HIPC(hipMemsetAsync(d.p, 'A', (size_t)L + 16, s));
    if (ch.end > ch.begin)
      h2d_host(d.p + ch.begin, seq + ch.begin, (size_t)(ch.end - ch.begin), s);
    q->parts[i] = query_device(
        use, d.p,
        checked(query_call_range((size_t)L, whole.k, w.begin, w.end)).with_max_occ(whole.max_occ),
        s);
    HIPC(hipStreamSynchronize(s));
  });
  if (bad.code != KMHG_OK) {
    free_query(q.release());
    fail(bad.code, bad.msg);
  }
  std::vector<int64_t> rows;
  for (auto* p : q->parts) rows.push_back(p->H);
  q->H = part_offsets(rows, q->part_off);
  return q.release();
}

// The rows of a multi-device query on its home device (peer copies, once), for the readers
// that want one device buffer (kmhg_query_rows_device).
void gather_parts(kmhg_query* q) {
  if (q->parts.empty() || q->gathered) return;
  DeviceGuard g(q->device);
  hipStream_t s = lib_stream();
  q->rows.reset((size_t)std::max<int64_t>(q->H, 1));
  for (size_t i = 0; i < q->parts.size(); ++i)
    if (q->parts[i]->H)
      HIPC(hipMemcpyPeerAsync(q->rows.p + q->part_off[i], q->device, q->parts[i]->rows.p,
                              q->parts[i]->device, (size_t)q->parts[i]->H * 8, s));
  HIPC(hipStreamSynchronize(s));
  q->stream = s;
  q->gathered = true;
}

void free_query(kmhg_query* q) {
  if (!q) return;
  for (auto* p : q->parts) free_query(p);
  DeviceGuard g(q->device);
  // the caller keeps its stream alive until here (a multi-device query's own rows exist only
  // once gathered, on the library stream)
  if (q->parts.empty() || q->gathered) HIPC(hipStreamSynchronize(q->stream));
  q->rows.ordered = false;                 // its stream is idle: straight back to the pool
  delete q;
}

void free_index(kmhg_index* idx) {
  if (!idx) return;
  for (auto& kv : idx->replicas) free_index(kv.second);
  idx->replicas.clear();
  DeviceGuard g(idx->device);
  // stream-ordered release: the buffers return to the pool once work queued on the index's
  // last stream has finished (queries on other streams are synchronised by their callers)
  ReleaseGroup rg(idx->stream);
  if (idx->pending) {                  // never used: no need to wait, the record is recycled
    // only the build has touched the buffers, and its event is already behind it: no second one
    rg.adopt(idx->rec.ev);
    PinnedPool::get().give(idx->rec, true);   // once the build's event has completed
    idx->pending = false;
  }
  idx->bind_all(idx->stream);
  delete idx;
}

}  // namespace

bool kmhg::ballot_ranks() { return lane_ballot(); }

// make.kmer.hash over a host string, synchronous like make_kmer_h_index: the checks and the copy
// of both host-string entries, `build` being build_device or its sampled form.
template <class Build>
void build_host_string(const char* seq, size_t L, int k, kmhg_index** out, Build&& build) {
  // small or refused strings: the C length and the checks before anything touches the device
  if (L < H2D_SCAN_MIN || k < 1 || k > 32 || L >= (size_t)INT32_MAX) {
    L = effective_len(seq, L);
    check_build_args(L, k);
  }
  hipStream_t s = lib_stream();
  DBuf<uint8_t> d(L + 16, s);
  L = h2d_cstring(d.p, seq, L, s);
  check_build_args(L, k);
  std::unique_ptr<kmhg_index> idx(build(d.p, (int64_t)L, s));
  finish_build(idx.get());   // (and d dies here)
  *out = idx.release();
}

// ============================================================================ C-ABI
extern "C" {

const char* kmhg_last_error(void) { return g_err.c_str(); }
int kmhg_version(void) { return 1; }

int kmhg_build(const char* seq, size_t L, int k, int do_sort, kmhg_index** out) {
  (void)do_sort;
  return guarded([&] {
    if (!seq || !out) fail(KMHG_EINVAL, "null argument");
    build_host_string(seq, L, k, out, [&](const uint8_t* d, int64_t n, hipStream_t s) {
      return build_device(d, n, k, s);
    });
  });
}

int kmhg_build_device(const void* d_seq, size_t L, int k, int do_sort, void* stream,
                      kmhg_index** out) {
  (void)do_sort;
  return guarded([&] {
    if (!d_seq || !out) fail(KMHG_EINVAL, "null argument");
    check_build_args(L, k);
    hipStream_t s = (hipStream_t)stream;   // caller stream; NULL = HIP null stream
    *out = build_device((const uint8_t*)d_seq, (int64_t)L, k, s);
  });
}

int kmhg_build_sampled(const char* seq, size_t L, int k, int w, int do_sort, kmhg_index** out) {
  (void)do_sort;
  return guarded([&] {
    if (!seq || !out) fail(KMHG_EINVAL, "null argument");
    check_sampling_args(k, w);
    build_host_string(seq, L, k, out, [&](const uint8_t* d, int64_t n, hipStream_t s) {
      return build_device_sampled(d, n, k, w, s);
    });
  });
}

int kmhg_build_sampled_device(const void* d_seq, size_t L, int k, int w, int do_sort,
                              void* stream, kmhg_index** out) {
  (void)do_sort;
  return guarded([&] {
    if (!d_seq || !out) fail(KMHG_EINVAL, "null argument");
    check_sampling_args(k, w);
    check_build_args(L, k);
    *out = build_device_sampled((const uint8_t*)d_seq, (int64_t)L, k, w, (hipStream_t)stream);
  });
}

int kmhg_get_sampling(const kmhg_index* idx, int* w) {
  return guarded([&] {
    if (!idx || !w) fail(KMHG_EINVAL, "null argument");
    *w = idx->sampling;
  });
}

int kmhg_minimizer_mask_device(const void* d_seq, size_t L, int k, int w, int rc,
                               uint32_t* d_mask_words, void* stream, int64_t* n_selected) {
  return guarded([&] {
    if (!d_seq || !d_mask_words || !n_selected) fail(KMHG_EINVAL, "null argument");
    check_sampling_args(k, w);
    check_query_args(L, k);
    *n_selected = minimizer_mask_device((const uint8_t*)d_seq, (int64_t)L, k, w, rc != 0,
                                        d_mask_words, (hipStream_t)stream);
  });
}

int kmhg_minimizer_mask(const char* seq, size_t L, int k, int w, int rc, uint8_t* mask) {
  return guarded([&] {
    if (!seq || !mask) fail(KMHG_EINVAL, "null argument");
    check_sampling_args(k, w);
    L = effective_len(seq, L);
    check_query_args(L, k);
    if (minimizer_mask_host((const uint8_t*)seq, (int64_t)L, k, w, rc != 0, mask) < 0)
      fail(KMHG_EINVAL, "w must be between 1 and 256");
  });
}

int kmhg_build_device_part(const void* d_seq, size_t L, int k, int part, int n_parts,
                           void* stream, kmhg_index** out) {
  return guarded([&] {
    if (!d_seq || !out) fail(KMHG_EINVAL, "null argument");
    check_build_args(L, k);
    if (n_parts < 1 || part < 0 || part >= n_parts) fail(KMHG_EINVAL, "part out of range");
    if (const char* e = test_build_knob("KMHG_BUILD"))
      if (std::string(e) == "v1") fail(KMHG_EINVAL, "part builds need the partitioned build");
    hipStream_t s = (hipStream_t)stream;
    *out = build_device_v2(
        BuildRequest::sequence_part((int64_t)L, k, (uint32_t)part, (uint32_t)n_parts),
        StreamPtrs{(const uint8_t*)d_seq, nullptr}, s);
  });
}

int kmhg_part_info(kmhg_index* idx, int64_t info[10]) {
  return guarded([&] {
    if (!idx || !info) fail(KMHG_EINVAL, "null argument");
    if (!idx->is_part) fail(KMHG_EINVAL, "not a part index");
    DeviceGuard g(idx->device);
    finish_build(idx);
    const Geom& G = idx->geom;
    const uint32_t side_b = side_bucket_of(G.nbh);
    info[0] = G.b0;
    info[1] = G.nb;
    info[2] = G.nbh;
    info[3] = G.capb;
    info[4] = (int64_t)idx->N;
    info[5] = (int64_t)idx->U;
    info[6] = (int64_t)idx->P;
    info[7] = idx->max_n;
    info[8] = (G.nb && side_b >= G.b0 && side_b < G.b0 + G.nb) ? 1 : 0;
    info[9] = idx->dcodes.p ? (int64_t)(diag_block_words(idx->L - idx->k + 1) * 8) : 0;
  });
}

int kmhg_part_export(kmhg_index* idx, int64_t pos_base, void* d_table, void* d_side_slot,
                     void* d_positions, void* d_codes, void* stream) {
  return guarded([&] {
    if (!idx) fail(KMHG_EINVAL, "null index");
    if (!idx->is_part) fail(KMHG_EINVAL, "not a part index");
    if (pos_base < 0 || pos_base + (int64_t)idx->N > (int64_t)UINT32_MAX)
      fail(KMHG_EINVAL, "position base out of range");
    DeviceGuard g(idx->device);
    finish_build(idx);
    hipStream_t s = (hipStream_t)stream;
    const uint64_t n = (uint64_t)idx->geom.nb * idx->geom.capb;
    if (d_table && n)
      LAUNCH("k_part_rebase", s,
             launch_part_rebase(idx->table.p, static_cast<Slot*>(d_table), n,
                                (uint32_t)pos_base, s));
    if (d_side_slot && idx->geom.nb)
      LAUNCH("k_part_rebase", s,
             launch_part_rebase(idx->table.p + n, static_cast<Slot*>(d_side_slot), 1,
                                (uint32_t)pos_base, s));
    if (d_positions && idx->N)
      HIPC(hipMemcpyAsync(d_positions, idx->positions.p, idx->N * 4, hipMemcpyDeviceToDevice, s));
    if (d_codes && idx->dcodes.p)
      HIPC(hipMemcpyAsync(d_codes, idx->dcodes.p, diag_block_words(idx->L - idx->k + 1) * 8,
                          hipMemcpyDeviceToDevice, s));
    HIPC(hipStreamSynchronize(s));
  });
}

int kmhg_free(kmhg_index* idx) {
  return guarded([&] { free_index(idx); });
}

// count.kmers: windows never span two sequences of the character vector, so a batch is the
// sequences joined by 'N'.  Alone, a sequence's final N-free run of exactly k chars yields no
// window (init_kmer reaches the string's end, src/kmer_hash.c:235-237); followed by the 'N' it
// would, so such a run is left out of the batch.
constexpr size_t COUNT_BATCH = (size_t)1 << 30;   // chars per build

kmhg_index* new_counts_index(int k, int source_n) {
  auto idx = std::make_unique<kmhg_index>();
  HIPC(hipGetDevice(&idx->device));
  idx->k = k;
  idx->sources = (uint32_t)source_n;
  idx->stream = lib_stream();
  return idx.release();
}

void check_count_args(int64_t n_seqs, int k, int source, int source_n, kmhg_index* c) {
  // count_kmers, src/kmer_hash.c:549-563 and 579-581 (same order, same texts)
  if (n_seqs < 1) fail(KMHG_EINVAL, "seq_r should be a character vector of length at least one");
  if (k < 1 || k > 32) fail(KMHG_EINVAL, "k must be a positive integer less than 1+MAX_K");
  if (source_n < 1 || source >= source_n)
    fail(KMHG_EINVAL, "source_n must be larger than 1 and larger than source");
  if (!c) return;
  if (!c->sources || c->canonical)
    fail(KMHG_EINVAL, "count.kmers needs a counts pointer (one made by count.kmers)");
  if (c->k != k)
    fail(KMHG_EINVAL, "mismatch between specified k and that given in the external pointer");
  if ((uint32_t)source_n != c->sources)
    fail(KMHG_EINVAL, "source_n differs from the source_n the counts pointer was made with");
}

int kmhg_count(kmhg_index** idx, const char* const* seqs, const size_t* lens, int64_t n_seqs,
               int k, int source, int source_n) {
  return guarded([&] {
    if (!idx || (n_seqs > 0 && (!seqs || !lens))) fail(KMHG_EINVAL, "null argument");
    check_count_args(n_seqs, k, source, source_n, *idx);
    std::unique_ptr<kmhg_index> fresh;
    kmhg_index* c = *idx;
    if (!c) {
      fresh.reset(new_counts_index(k, source_n));
      c = fresh.get();
    }
    DeviceGuard g(c->device);
    if (source >= 0) {   // negative: every insert fails its source check, nothing is counted
      hipStream_t s = lib_stream();
      std::vector<char> buf;
      auto flush = [&] {
        if (buf.empty()) return;
        if (buf.size() >= (size_t)INT32_MAX)
          fail(KMHG_EOVERFLOW, "sequence longer than 2^31-1 (int positions)");
        DBuf<uint8_t> d(buf.size() + 16, s);
        HIPC(hipMemcpyAsync(d.p, buf.data(), buf.size(), hipMemcpyHostToDevice, s));
        count_device(c, d.p, (int64_t)buf.size(), (uint32_t)source, s);
        HIPC(hipStreamSynchronize(s));   // buf is reused
        buf.clear();
      };
      for (int64_t i = 0; i < n_seqs; ++i) {
        const char* q = seqs[i];
        if (!q) continue;
        size_t n = effective_len(q, lens[i]);
        if ((int64_t)n <= k) continue;                  // src/kmer_hash.c:583-584
        bool tail_k = LCN(q[n - k - 1]);                // final run of exactly k chars?
        for (size_t j = n - k; tail_k && j < n; ++j) tail_k = !LCN(q[j]);
        if (tail_k) n -= (size_t)k;
        if (!buf.empty() && buf.size() + n + 1 > COUNT_BATCH) flush();
        buf.insert(buf.end(), q, q + n);
        buf.push_back('N');
      }
      flush();
    }
    if (fresh) *idx = fresh.release();
  });
}

int kmhg_count_device(kmhg_index** idx, const void* d_seq, size_t L, int k, int source,
                      int source_n, void* stream) {
  return guarded([&] {
    if (!idx || (L && !d_seq)) fail(KMHG_EINVAL, "null argument");
    check_count_args(1, k, source, source_n, *idx);
    if (L >= (size_t)INT32_MAX) fail(KMHG_EOVERFLOW, "sequence longer than 2^31-1 (int positions)");
    std::unique_ptr<kmhg_index> fresh;
    kmhg_index* c = *idx;
    if (!c) {
      fresh.reset(new_counts_index(k, source_n));
      c = fresh.get();
    }
    DeviceGuard g(c->device);
    if (source >= 0) count_device(c, (const uint8_t*)d_seq, (int64_t)L, (uint32_t)source,
                                  (hipStream_t)stream);
    if (fresh) *idx = fresh.release();
  });
}

// ---------------------------------------------------------------- suffix hash (read counting)
// count_kmers_fastq_sh_rp (src/kmer_hash.c:810-857) and count_kmers_fastq_sh (:715-806), whose
// suffix_hash (one count per canonical k-mer) is a suffix hash of one source with `single` set
// (info.kind = 3); the two pointer kinds refuse each other as the reference's tags do.  A call's
// parameter vector is decoded by read_call_rp / read_call_sh1 (kmhg_reads.h: a ReadCall); one
// body per input kind then serves both.
struct kmhg_reads {
  ReadsHost r;
};

// A call's first refusals, in each entry's order: .rp looks at the kind of a given pointer before
// its parameters, the single suffix hash after them (ReadTarget).
static void check_read_call(const kmhg_index* given, const ReadCall& call) {
  if (given && !call.single) check_sh(given);
  if (call.err) fail(call.err, call.msg);
}

// The suffix hash a call counts into: the given one, or a fresh one that *sh receives only once
// the count has succeeded (publish).  c == nullptr: count nothing -- into an existing suffix
// hash the reference's .rp checks k and source (src/kmer_reader.c:118-126), and a mismatch
// prints a message and counts nothing.  A single suffix hash refuses instead.
namespace {
struct ReadTarget {
  kmhg_index* c = nullptr;
  std::unique_ptr<kmhg_index> fresh;
  ReadTarget(kmhg_index* given, const ReadCall& call, hipStream_t s) {
    if (!given) {
      fresh.reset(new_sh_index(call.k, (int)call.sources, s));
      fresh->single = call.single;
      c = fresh.get();
    } else if (call.single) {
      if (!given->canonical || !given->single)
        fail(KMHG_EINVAL, "Unable to extract suffix_hash from external pointer");
      if (given->k != call.k) fail(KMHG_EINVAL, "k differs from the k of the suffix hash");
      c = given;
    } else if ((int)given->k != call.k) {
      fprintf(stderr, "Incompatible arguments: k and total bit numbers do not add up\n");
    } else if (call.walk.source >= given->sources) {
      fprintf(stderr, "Value of source is too large\n");
    } else {
      c = given;
    }
  }
  void publish(kmhg_index** sh) { if (fresh) *sh = fresh.release(); }
};
}  // namespace

static void count_fastq(kmhg_index** sh, const char* path, const ReadCall& call) {
  check_read_call(*sh, call);
  hipStream_t s = lib_stream();
  ReadTarget t(*sh, call, s);
  if (!t.c) return;
  DeviceGuard g(t.c->device);
  ReadsHost r;
  const auto count = [&](ReadsHost& b) { sh_count_reads_host(t.c, b, call.walk, s); };
  read_fastx(path, call.max_reads, call.k, r, count);
  count(r);
  t.publish(sh);
}

static void count_reads(kmhg_index** sh, const kmhg_reads* r, const ReadCall& call) {
  check_read_call(*sh, call);
  hipStream_t s = lib_stream();
  ReadTarget t(*sh, call, s);
  if (!t.c) return;
  DeviceGuard g(t.c->device);
  ReadsHost keep;
  sh_count_reads_host(t.c, *reads_longer_than(r->r, call.k, keep), call.walk, s);
  t.publish(sh);
}

// Device-resident packed reads.  A device batch's key stream is sized by per-read window bounds
// (each <= the read's length) summed in u32: a batch spanning 2^32 or more bases could wrap that
// sum (batch_span_ok, from two int64 reads).
static void count_reads_device(kmhg_index** sh, const void* d_seq, const void* d_qual,
                               const int64_t* d_offsets, const uint8_t* d_has_qual,
                               int64_t n_reads, const ReadCall& call, hipStream_t s) {
  if (n_reads > 0 && (!d_seq || !d_qual || !d_offsets || !d_has_qual))
    fail(KMHG_EINVAL, "null argument");
  check_read_call(*sh, call);
  if (n_reads < 0 || n_reads >= (int64_t)UINT32_MAX) fail(KMHG_EINVAL, "bad read count");
  if ((reinterpret_cast<uintptr_t>(d_seq) | reinterpret_cast<uintptr_t>(d_qual)) & 15)
    fail(KMHG_EINVAL, "read bases and qualities must be 16-byte aligned");
  ReadTarget t(*sh, call, s);
  if (!t.c) return;
  DeviceGuard g(t.c->device);
  if (n_reads > 0) {
    int64_t ends[2] = {0, 0};
    HIPC(hipMemcpyAsync(&ends[0], d_offsets, 8, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(&ends[1], d_offsets + n_reads, 8, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    if (!batch_span_ok(ends[0], ends[1]))
      fail(KMHG_EINVAL, "a read batch must span fewer than 2^32 bases: split it");
  }
  sh_count_reads_device(t.c, (const uint8_t*)d_seq, (const uint8_t*)d_qual, d_offsets,
                        d_has_qual, (uint32_t)n_reads, call.walk, s);
  t.publish(sh);
}

int kmhg_sh_count_fastq(kmhg_index** sh, const char* path, const int32_t params[8]) {
  return guarded([&] {
    if (!sh || !path || !params) fail(KMHG_EINVAL, "null argument");
    count_fastq(sh, path, read_call_rp(params));
  });
}

int kmhg_fastx_read(const char* path, int64_t max_reads, int k, kmhg_reads** out) {
  return guarded([&] {
    if (!path || !out) fail(KMHG_EINVAL, "null argument");
    auto r = std::make_unique<kmhg_reads>();
    read_fastx(path, (uint64_t)max_reads, k, r->r, nullptr);
    *out = r.release();
  });
}

int kmhg_reads_info(const kmhg_reads* r, int64_t* n_records, int64_t* n_reads,
                    int64_t* n_bases) {
  return guarded([&] {
    if (!r) fail(KMHG_EINVAL, "null argument");
    if (n_records) *n_records = r->r.records;
    if (n_reads) *n_reads = (int64_t)r->r.n();
    if (n_bases) *n_bases = (int64_t)r->r.seq.size();
  });
}

int kmhg_reads_copy(const kmhg_reads* r, uint8_t* seq, uint8_t* qual, int64_t* offsets,
                    uint8_t* has_qual) {
  return guarded([&] {
    if (!r) fail(KMHG_EINVAL, "null argument");
    const ReadsHost& h = r->r;
    if (seq) memcpy(seq, h.seq.data(), h.seq.size());
    if (qual) memcpy(qual, h.qual.data(), h.qual.size());
    if (offsets) memcpy(offsets, h.off.data(), h.off.size() * 8);
    if (has_qual) memcpy(has_qual, h.hasq.data(), h.hasq.size());
  });
}

int kmhg_reads_free(kmhg_reads* r) {
  delete r;
  return KMHG_OK;
}

int kmhg_sh_count_reads(kmhg_index** sh, const kmhg_reads* r, const int32_t params[8]) {
  return guarded([&] {
    if (!sh || !r || !params) fail(KMHG_EINVAL, "null argument");
    count_reads(sh, r, read_call_rp(params));
  });
}

int kmhg_sh_count_reads_device(kmhg_index** sh, const void* d_seq, const void* d_qual,
                               const int64_t* d_offsets, const uint8_t* d_has_qual,
                               int64_t n_reads, const int32_t params[8], void* stream) {
  return guarded([&] {
    if (!sh || !params) fail(KMHG_EINVAL, "null argument");
    count_reads_device(sh, d_seq, d_qual, d_offsets, d_has_qual, n_reads, read_call_rp(params),
                       (hipStream_t)stream);
  });
}

// The single suffix hash: params = (k, report_n, prefix_bits, max_memory, min_quality,
// max_read_n); the deviations on the reference's undefined paths are listed in kmhgpu.h.
int kmhg_sh1_count_fastq(kmhg_index** sh, const char* path, const int32_t params[6]) {
  return guarded([&] {
    if (!sh || !path || !params) fail(KMHG_EINVAL, "null argument");
    count_fastq(sh, path, read_call_sh1(params));
  });
}

int kmhg_sh1_count_reads(kmhg_index** sh, const kmhg_reads* r, const int32_t params[6]) {
  return guarded([&] {
    if (!sh || !r || !params) fail(KMHG_EINVAL, "null argument");
    count_reads(sh, r, read_call_sh1(params));
  });
}

int kmhg_sh1_count_reads_device(kmhg_index** sh, const void* d_seq, const void* d_qual,
                                const int64_t* d_offsets, const uint8_t* d_has_qual,
                                int64_t n_reads, const int32_t params[6], void* stream) {
  return guarded([&] {
    if (!sh || !params) fail(KMHG_EINVAL, "null argument");
    count_reads_device(sh, d_seq, d_qual, d_offsets, d_has_qual, n_reads, read_call_sh1(params),
                       (hipStream_t)stream);
  });
}

// k_spectrum over sh's rows into counts (nbins doubles, zeroed by the caller): args holds comb_n
// combinations, their comb_n inner flags and one source_min per source.
static void spectrum_bins(kmhg_index* sh, uint32_t max_count, const std::vector<uint32_t>& args,
                          uint32_t comb_n, size_t nbins, double* counts) {
  DeviceGuard g(sh->device);
  hipStream_t s = lib_stream();
  finish_build(sh);
  if (!sh->U) return;
  DBuf<uint32_t> dargs(args.size(), s), bins(nbins, s);
  HIPC(hipMemcpyAsync(dargs.p, args.data(), args.size() * 4, hipMemcpyHostToDevice, s));
  HIPC(hipMemsetAsync(bins.p, 0, nbins * 4, s));
  LAUNCH("k_spectrum", s,
         launch_spectrum(sh->positions.p, sh->U, sh->sources, max_count, dargs.p, dargs.p + comb_n,
                         comb_n, dargs.p + 2 * comb_n, bins.p, s));
  std::vector<uint32_t> h(nbins);
  HIPC(hipMemcpyAsync(h.data(), bins.p, nbins * 4, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  for (size_t i = 0; i < nbins; ++i) counts[i] = (double)h[i];
}

// sh_count_spectrum (src/suffix_hash.c:112-129): counts[min(count, max_count)] += 1 per k-mer.
// k_spectrum's bins for one source, one combination {1} (not inner) and source_min 0 are the
// same sum: every row's flag is 1, so bin min(count, max_count) gains one per row.
int kmhg_sh1_spectrum(kmhg_index* sh, int max_count, double* counts) {
  return guarded([&] {
    if (!sh || !sh->canonical || !sh->single)
      fail(KMHG_EINVAL, "unable to obtain a suffix_hash from external pointer");
    if (max_count < 1 || max_count > (1 << 30)) fail(KMHG_EINVAL, "Unsuitable value of max_count");
    if (!counts) fail(KMHG_EINVAL, "null argument");
    const size_t nbins = (size_t)max_count + 1;
    std::fill(counts, counts + nbins, 0.0);
    spectrum_bins(sh, (uint32_t)max_count, {1u, 0u, 0u}, 1, nbins, counts);
  });
}

// seq_kmer_depth_sh (src/kmer_hash.c:859-879) + seq_kmer_counts (src/kmer_reader.c:155-193)
static void check_depth(const kmhg_index* sh, int k) {
  check_sh(sh);
  if (k != sh->k) fail(KMHG_EINVAL, "Receieved error from seq_kmer_counts");
}

int kmhg_sh_depth(kmhg_index* sh, const char* seq, size_t L, int k, int32_t* counts) {
  return guarded([&] {
    check_depth(sh, k);
    if (L && (!seq || !counts)) fail(KMHG_EINVAL, "null argument");
    if (L >= (size_t)INT32_MAX) fail(KMHG_EOVERFLOW, "sequence longer than 2^31-1");
    DeviceGuard g(sh->device);
    hipStream_t s = lib_stream();
    const size_t n = effective_len(seq, L);     // the walk ends at a NUL
    const size_t S = sh->sources;
    DBuf<uint8_t> d(n + 16, s);
    DBuf<int32_t> out(std::max<size_t>(L * S, 1), s);
    if (n) HIPC(hipMemcpyAsync(d.p, seq, n, hipMemcpyHostToDevice, s));
    sh_depth_device(sh, d.p, (int64_t)n, k, out.p, s);
    if (L > n)   // past a NUL: never written (NA)
      HIPC(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out.p + n * S), (int)INT_MIN,
                             (L - n) * S, s));
    if (L) d2h_host(counts, out.p, L * S * 4, s);
    HIPC(hipStreamSynchronize(s));
  });
}

int kmhg_sh_depth_device(kmhg_index* sh, const void* d_seq, size_t L, int k, int32_t* d_counts,
                         void* stream) {
  return guarded([&] {
    check_depth(sh, k);
    if (L && (!d_seq || !d_counts)) fail(KMHG_EINVAL, "null argument");
    if (L >= (size_t)INT32_MAX) fail(KMHG_EOVERFLOW, "sequence longer than 2^31-1");
    DeviceGuard g(sh->device);
    sh_depth_device(sh, (const uint8_t*)d_seq, (int64_t)L, k, d_counts, (hipStream_t)stream);
  });
}

// kmer_spectrum_suffix_hash_n (src/kmer_hash.c:1010-1039) + sh_count_spectrum_nc
// (src/suffix_hash.c:338-421).  *status = 1, or the reference's negative code (counts zero).
int kmhg_sh_spectrum(kmhg_index* sh, int max_count, const int32_t* comb,
                     const int32_t* comb_inner, int comb_n, const int32_t* source_min,
                     int n_source_min, double* counts, int* status) {
  return guarded([&] {
    check_sh(sh);
    if (comb_n < 1) fail(KMHG_EINVAL, "comb_r should be an integer vector of length > 0");
    if (!comb || !comb_inner)
      fail(KMHG_EINVAL, "comb_inner_r should be an integer vector of the same length as comb_r");
    if (n_source_min != (int)sh->sources || !source_min)
      fail(KMHG_EINVAL, "source_min_r should be an integer vector of length sh->counts_n");
    if (max_count < 0) fail(KMHG_EINVAL, "max_count must be >= 0");   // reference: R alloc error
    if (!counts) fail(KMHG_EINVAL, "null argument");
    const uint32_t S = sh->sources;
    const size_t nbins = (size_t)(max_count + 1) * (size_t)comb_n * S;
    std::fill(counts, counts + nbins, 0.0);
    const int st = spectrum_status(comb, comb_inner, comb_n, S);
    if (status) *status = st;
    if (st != 1) {
      fprintf(stderr, "sh_count_spectrum_nc returned an error: %d\n", st);
      return;
    }
    std::vector<uint32_t> args((size_t)2 * comb_n + S);
    for (int i = 0; i < comb_n; ++i) {
      args[i] = (uint32_t)comb[i];
      args[comb_n + i] = (uint32_t)comb_inner[i];
    }
    for (uint32_t j = 0; j < S; ++j) args[2 * comb_n + j] = (uint32_t)source_min[j];
    spectrum_bins(sh, (uint32_t)max_count, args, (uint32_t)comb_n, nbins, counts);
  });
}

// (key, counts) rows of a counts index in row order (tests, export)
int kmhg_counts_export(kmhg_index* idx, uint64_t* keys, int32_t* counts) {
  return guarded([&] {
    if (!idx || !idx->sources) fail(KMHG_EINVAL, "not a counts index");
    DeviceGuard g(idx->device);
    hipStream_t s = lib_stream();
    idx->stream = s;
    ReleaseGroup rg(s);
    ensure_row_order(idx, s);
    const uint64_t U = idx->U, S = idx->sources;
    const uint64_t* k = idx->ckeys.p;
    const int32_t* m = idx->positions.p;
    DBuf<uint64_t> gk;
    DBuf<int32_t> gm;
    if (U && row_order_of(idx) && (keys || counts)) {   // rows in first-insertion order
      gk.reset(U);
      gm.reset(U * S);
      gk.bind(s);
      gm.bind(s);
      LAUNCH("k_rows_gather", s, launch_rows_gather(row_order_of(idx), idx->ckeys.p,
                                                    idx->positions.p, (uint32_t)U, (uint32_t)S,
                                                    gk.p, gm.p, s));
      k = gk.p;
      m = gm.p;
    }
    if (U && keys) HIPC(hipMemcpyAsync(keys, k, U * 8, hipMemcpyDeviceToHost, s));
    if (U && counts) HIPC(hipMemcpyAsync(counts, m, U * S * 4, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
  });
}

int kmhg_sh_last_batch(const kmhg_index* sh, double* distinct_est, int* spread, int* path) {
  return guarded([&] {
    if (!sh || !sh->canonical) fail(KMHG_EINVAL, "not a suffix hash");
    if (distinct_est) *distinct_est = sh->co_est;
    if (spread) *spread = sh->co_spread;
    if (path) *path = sh->co_path;
  });
}

int kmhg_index_wait(kmhg_index* idx) {
  return guarded([&] {
    if (!idx) fail(KMHG_EINVAL, "null index");
    DeviceGuard g(idx->device);
    finish_build(idx);
  });
}

int kmhg_index_info(const kmhg_index* cidx, kmhg_info* info) {
  return guarded([&] {
    if (!cidx || !info) fail(KMHG_EINVAL, "null argument");
    kmhg_index* idx = const_cast<kmhg_index*>(cidx);   // completes a pending build
    DeviceGuard g(idx->device);
    finish_build(idx);
    info->k = idx->k;
    info->device = idx->device;
    info->seq_len = idx->L;
    info->n_kmers = (int64_t)idx->U;
    info->n_positions = (int64_t)idx->N;
    info->n_pairs = (int64_t)idx->P;
    info->max_count = idx->max_n;
    info->table_slots = (int64_t)idx->slots();
    info->device_bytes = (int64_t)(idx->table.bytes() + idx->positions.bytes() +
                                   idx->ckeys.bytes() + idx->slot_row.bytes() +
                                   idx->row_slot.bytes());
    info->sources = (int32_t)idx->sources;
    info->kind = idx->single ? 3 : idx->canonical ? 2 : (idx->sources ? 1 : 0);
    info->kmer_count = (int64_t)(idx->sources ? idx->kmer_count : idx->U);
    info->build = idx->build_kind;
    info->fallback = idx->fallback;
  });
}

int kmhg_set_row_order(kmhg_index* idx, int order) {
  return guarded([&] {
    if (!idx) fail(KMHG_EINVAL, "null index");
    if (order != KMHG_ORDER_FIRST && order != KMHG_ORDER_KHASH) fail(KMHG_EINVAL, "unknown row order");
    idx->row_order = order;
  });
}

int kmhg_set_max_occ(kmhg_index* idx, int64_t max_occ) {
  return guarded([&] {
    if (!idx) fail(KMHG_EINVAL, "null index");
    checked(max_occ_refusal(max_occ));
    if (idx->canonical || idx->single) fail(KMHG_EINVAL, "External pointer has incorrect tag");
    if (idx->sources) fail(KMHG_EINVAL, "max.occ needs a position index");
    idx->max_occ.store(max_occ, std::memory_order_relaxed);
  });
}

int kmhg_get_max_occ(const kmhg_index* idx, int64_t* max_occ) {
  return guarded([&] {
    if (!idx || !max_occ) fail(KMHG_EINVAL, "null argument");
    *max_occ = idx->max_occ.load(std::memory_order_relaxed);
  });
}

int kmhg_khash_order(const uint64_t* keys, int64_t n, uint32_t* order) {
  return guarded([&] {
    if (n < 0 || (n && (!keys || !order))) fail(KMHG_EINVAL, "null argument");
    const std::vector<uint64_t> k(keys, keys + n);
    const std::vector<uint32_t> o = khash_bucket_order(k);
    std::copy(o.begin(), o.end(), order);
  });
}

int kmhg_get_row_order(const kmhg_index* idx, int* order) {
  return guarded([&] {
    if (!idx || !order) fail(KMHG_EINVAL, "null argument");
    *order = idx->row_order;
  });
}

int kmhg_positions_size(kmhg_index* idx, uint32_t opt, int64_t* n_kmers, int64_t* n_pos_rows,
                        int64_t* n_pair_rows, int64_t* n_counts) {
  return guarded([&] {
    if (!idx) fail(KMHG_EINVAL, "null index");
    DeviceGuard g(idx->device);
    finish_build(idx);
    positions_sizes(idx, opt, n_kmers, n_pos_rows, n_pair_rows, n_counts);
  });
}

int kmhg_positions_fill_device(kmhg_index* idx, uint32_t opt, char* d_kmers, int32_t* d_pos,
                               int32_t* d_pairs, int32_t* d_counts, void* stream) {
  return guarded([&] {
    if (!idx) fail(KMHG_EINVAL, "null index");
    DeviceGuard g(idx->device);
    hipStream_t s = (hipStream_t)stream;   // caller stream; NULL = HIP null stream
    positions_device(idx, opt, d_kmers, d_pos, d_pairs, d_counts, s);
  });
}

// kmer.pos's pair rows into a host matrix (the R API's readout) from HOST_PAIRS_MIN rows on: the
// lists and their keys' offsets cross PCIe and host threads write the rows (kmhg_hostwork.h).
// KMHG_HOST_PAIRS=0 (test build): the rows are made on the device and copied.
static_assert(sizeof(RowInfo) == sizeof(uint2), "RowInfo is copied straight from Canon::rinfo");
static void pairs_to_host(kmhg_index* idx, int32_t* out, hipStream_t s) {
  Canon& c = idx->canon;                     // prepare_readout ran (positions_device)
  const uint64_t M = c.n_multi, U = idx->U, P = idx->P;
  std::unique_ptr<uint32_t[]> pk(new uint32_t[M]);
  std::unique_ptr<uint64_t[]> po(new uint64_t[M]);
  std::unique_ptr<RowInfo[]> ri(new RowInfo[U]);
  d2h_host(pk.get(), c.pkeys.p, M * 4, s);
  d2h_host(po.get(), c.pair_off.p, M * 8, s);
  d2h_host(ri.get(), c.rinfo.p, U * 8, s);
  uint64_t n_lists = 0;                      // the list entries in use: [0, max end)
  for (uint64_t m = 0; m < M; ++m) n_lists = std::max<uint64_t>(n_lists, ri[pk[m]].y);
  if (n_lists > idx->positions.n) fail(KMHG_EDEVICE, "pair lists beyond the positions");
  std::unique_ptr<int32_t[]> ps(new int32_t[std::max<uint64_t>(n_lists, 1)]);
  d2h_host(ps.get(), idx->positions.p, n_lists * 4, s);
  hint_huge_pages(out, P * 12);
  expand_pairs_host(pk.get(), po.get(), M, ri.get(), ps.get(), P, out, expand_threads(P * 12),
                    fresh_threads());
}

int kmhg_positions_fill(kmhg_index* idx, uint32_t opt, char* kmers, int32_t* pos, int32_t* pairs,
                        int32_t* counts) {
  return guarded([&] {
    if (!idx) fail(KMHG_EINVAL, "null index");
    DeviceGuard g(idx->device);
    hipStream_t s = lib_stream();
    const size_t U = idx->U;
    const char* hpe = test_build_knob("KMHG_HOST_PAIRS");
    const bool host_pairs = (opt & KMHG_OPT_PAIRS) && pairs && idx->P >= HOST_PAIRS_MIN &&
                            idx->sources == 0 && !(hpe && hpe[0] == '0');   // position indices
    const uint32_t dopt = host_pairs ? opt & ~(uint32_t)KMHG_OPT_PAIRS : opt;
    DBuf<char> dk((opt & KMHG_OPT_KMER) ? U * (idx->k + 1) : 0, s);
    DBuf<int32_t> dp((opt & KMHG_OPT_POS) ? 2 * idx->N : 0, s);
    DBuf<int32_t> dpp((dopt & KMHG_OPT_PAIRS) ? 3 * idx->P : 0, s);
    DBuf<int32_t> dc((opt & KMHG_OPT_COUNT) ? U : 0, s);
    positions_device(idx, dopt, dk.p, dp.p, dpp.p, dc.p, s);
    if ((opt & KMHG_OPT_KMER) && U && kmers)
      d2h_host(kmers, dk.p, dk.bytes(), s);
    if ((opt & KMHG_OPT_POS) && idx->N && pos)
      d2h_host(pos, dp.p, dp.bytes(), s);
    if (host_pairs)
      pairs_to_host(idx, pairs, s);
    else if ((opt & KMHG_OPT_PAIRS) && idx->P && pairs)
      d2h_host(pairs, dpp.p, dpp.bytes(), s);
    if ((opt & KMHG_OPT_COUNT) && U && counts)
      d2h_host(counts, dc.p, dc.bytes(), s);
    HIPC(hipStreamSynchronize(s));
  });
}

int kmhg_pairs_run(kmhg_index* a, kmhg_index* b, kmhg_query** q, int64_t* n_rows) {
  return guarded([&] {
    if (!a || !b || !q) fail(KMHG_EINVAL, "null argument");
    DeviceGuard g(a->device);
    hipStream_t s = lib_stream();
    *q = pairs_device(a, b, s);
    HIPC(hipStreamSynchronize(s));
    if (n_rows) *n_rows = (*q)->H;
  });
}

int kmhg_pairs_run_device(kmhg_index* a, kmhg_index* b, void* stream, kmhg_query** q,
                          int64_t* n_rows) {
  return guarded([&] {
    if (!a || !b || !q) fail(KMHG_EINVAL, "null argument");
    DeviceGuard g(a->device);
    *q = pairs_device(a, b, (hipStream_t)stream);
    if (n_rows) *n_rows = (*q)->H;
  });
}

// The host-pointer entries (kmhg_query_run, kmhg_query_run_rc) on the index's device: the
// string goes up as it is -- the forward one for rc too, no reversed copy anywhere -- and the
// call is checked again at its C length.
static void query_host(kmhg_index* idx, const char* seq, size_t L, int k, bool rc, kmhg_query** q,
                       int64_t* n_rows) {
  if (L < H2D_SCAN_MIN || k < 1 || k > 31 || L >= (size_t)INT32_MAX) {
    L = effective_len(seq, L);             // (as kmhg_build)
    check_query_args(L, k);
  }
  DeviceGuard g(idx->device);
  hipStream_t s = lib_stream();
  DBuf<uint8_t> d(L + 16, s);
  L = h2d_cstring(d.p, seq, L, s);
  *q = query_device(idx, d.p, capped(idx, query_call(L, k)).on_rc(rc), s);
  HIPC(hipStreamSynchronize(s));
  if (n_rows) *n_rows = (*q)->H;
}

// The device-pointer entries: `c` names the query, `stream` is the caller's (NULL = HIP null
// stream).
static void query_entry(kmhg_index* idx, const void* d_seq, const QueryCall& c, void* stream,
                        kmhg_query** q, int64_t* n_rows, int64_t* n_runs = nullptr) {
  if (!idx || !d_seq || !q) fail(KMHG_EINVAL, "null argument");
  const QueryCall cc = capped(idx, c);
  DeviceGuard g(idx->device);
  *q = query_device(idx, static_cast<const uint8_t*>(d_seq), cc, (hipStream_t)stream);
  if (n_rows) *n_rows = (*q)->H;
  if (n_runs) *n_runs = (*q)->n_runs;
}

int kmhg_query_run(kmhg_index* idx, const char* seq, size_t L, int k, kmhg_query** q,
                   int64_t* n_rows) {
  return guarded([&] {
    if (!idx || !seq || !q) fail(KMHG_EINVAL, "null argument");
    const std::vector<int> devs = query_devices();
    if (devs.size() > 1 && idx->sources == 0) {   // position index over several devices
      *q = query_multi_device(idx, seq, capped(idx, query_call(effective_len(seq, L), k)), devs);
      if (n_rows) *n_rows = (*q)->H;
      return;
    }
    query_host(idx, seq, L, k, false, q, n_rows);
  });
}

int kmhg_query_run_device(kmhg_index* idx, const void* d_seq, size_t L, int k, void* stream,
                          kmhg_query** q, int64_t* n_rows) {
  return guarded([&] { query_entry(idx, d_seq, query_call(L, k), stream, q, n_rows); });
}

int kmhg_query_run_device_range(kmhg_index* idx, const void* d_seq, size_t L, int k,
                                int64_t w_begin, int64_t w_end, void* stream, kmhg_query** q,
                                int64_t* n_rows) {
  return guarded([&] {
    query_entry(idx, d_seq, query_call_range(L, k, w_begin, w_end), stream, q, n_rows);
  });
}

int kmhg_query_run_device_range_runs(kmhg_index* idx, const void* d_seq, size_t L, int k,
                                     int64_t w_begin, int64_t w_end, void* stream,
                                     kmhg_query** q, int64_t* n_rows, int64_t* n_runs) {
  return guarded([&] {
    query_entry(idx, d_seq, query_call_range(L, k, w_begin, w_end).as_runs(), stream, q, n_rows,
                n_runs);
  });
}

// The reverse strand (include/kmhgpu.h): the forward entries' checks and words, the forward
// sequence on the device, rc down to the probe's stage fill.
int kmhg_query_run_rc(kmhg_index* idx, const char* seq, size_t L, int k, kmhg_query** q,
                      int64_t* n_rows) {
  return guarded([&] {
    if (!idx || !seq || !q) fail(KMHG_EINVAL, "null argument");
    query_host(idx, seq, L, k, true, q, n_rows);
  });
}

int kmhg_query_run_rc_device_range(kmhg_index* idx, const void* d_seq, size_t L, int k,
                                   int64_t w_begin, int64_t w_end, void* stream, kmhg_query** q,
                                   int64_t* n_rows) {
  return guarded([&] {
    query_entry(idx, d_seq, query_call_range(L, k, w_begin, w_end).on_rc(), stream, q, n_rows);
  });
}

int kmhg_query_run_rc_device_range_runs(kmhg_index* idx, const void* d_seq, size_t L, int k,
                                        int64_t w_begin, int64_t w_end, void* stream,
                                        kmhg_query** q, int64_t* n_rows, int64_t* n_runs) {
  return guarded([&] {
    query_entry(idx, d_seq, query_call_range(L, k, w_begin, w_end).as_runs().on_rc(), stream, q,
                n_rows, n_runs);
  });
}

int kmhg_query_run_device_part(kmhg_index* part, const void* d_seq, size_t L, int k,
                               void* stream, kmhg_query** q, int64_t* n_rows) {
  return guarded([&] { query_entry(part, d_seq, query_call(L, k).of_part(), stream, q, n_rows); });
}

int kmhg_query_runs_device(kmhg_query* q, const int32_t** d_runs) {
  return guarded([&] {
    if (!q || !d_runs) fail(KMHG_EINVAL, "null argument");
    if (q->n_runs < 0) fail(KMHG_EINVAL, "the query holds rows, not runs");
    *d_runs = q->runs.p;
  });
}

int kmhg_query_tile_offsets(kmhg_query* q, uint64_t* d_out, int64_t* n_tiles, void* stream) {
  return guarded([&] {
    if (!q || !n_tiles) fail(KMHG_EINVAL, "null argument");
    if (!q->tile_off.p && q->H) fail(KMHG_EINVAL, "not a part query");
    *n_tiles = q->n_tiles;
    if (!d_out) return;
    DeviceGuard g(q->device);
    hipStream_t s = (hipStream_t)stream;
    if (q->n_tiles)
      HIPC(hipMemcpyAsync(d_out, q->tile_off.p, (size_t)q->n_tiles * 8, hipMemcpyDeviceToDevice, s));
    const uint64_t h = (uint64_t)q->H;            // [n_tiles] = the part's row total
    launch_fill_u64(d_out + q->n_tiles, h, s);
  });
}

int kmhg_merge_part_rows(const void* d_rows, const uint64_t* d_seg_base, const uint64_t* d_tile_off,
                         int n_parts, int64_t n_tiles, int k, int64_t w0, void* d_out,
                         void* stream) {
  return guarded([&] {
    if (n_parts < 1 || n_tiles < 0 || k < 1 || k > 32) fail(KMHG_EINVAL, "bad merge arguments");
    if (!n_tiles) return;
    if (!d_rows || !d_seg_base || !d_tile_off || !d_out) fail(KMHG_EINVAL, "null argument");
    hipStream_t s = (hipStream_t)stream;
    LAUNCH("k_merge_part_rows", s,
           launch_merge_part_rows(reinterpret_cast<const int2*>(d_rows), d_seg_base, d_tile_off,
                                  (uint32_t)n_parts, (uint32_t)n_tiles, k, w0,
                                  reinterpret_cast<int2*>(d_out), s));
    HIPC(hipGetLastError());
  });
}

int kmhg_part_first_mask(kmhg_index* part, uint32_t* d_mask, void* stream) {
  return guarded([&] {
    check_part_read(part);
    if (!d_mask) fail(KMHG_EINVAL, "null argument");
    DeviceGuard g(part->device);
    part_first_mask(part, d_mask, (hipStream_t)stream);
  });
}

int kmhg_part_positions_size(kmhg_index* part, uint32_t opt, int64_t* n_kmers,
                             int64_t* n_pos_rows, int64_t* n_pair_rows) {
  return guarded([&] {
    check_part_read(part);
    DeviceGuard g(part->device);
    finish_build(part);
    if (n_kmers) *n_kmers = (int64_t)part->U;
    if (n_pos_rows) *n_pos_rows = (opt & KMHG_OPT_POS) ? (int64_t)part->N : 0;
    if (n_pair_rows) *n_pair_rows = (opt & KMHG_OPT_PAIRS) ? (int64_t)part->P : 0;
  });
}

int kmhg_part_positions_fill_device(kmhg_index* part, const uint32_t* d_global_mask, uint32_t opt,
                                    int32_t* d_labels, char* d_kmers, int32_t* d_pos,
                                    int32_t* d_pairs, int32_t* d_counts, void* stream) {
  return guarded([&] {
    check_part_read(part);
    DeviceGuard g(part->device);
    part_positions_device(part, d_global_mask, opt, d_labels, d_kmers, d_pos, d_pairs, d_counts,
                          (hipStream_t)stream);
  });
}

int kmhg_merge_part_positions(int n_parts, uint32_t opt, int k, const int64_t* n_kmers,
                              const int64_t* n_pos_rows, const int64_t* n_pair_rows,
                              const int32_t* const* d_labels, const int32_t* const* d_counts,
                              const char* const* d_kmers, const int32_t* const* d_pos,
                              const int32_t* const* d_pairs, char* d_out_kmers,
                              int32_t* d_out_pos, int32_t* d_out_pairs, int32_t* d_out_counts,
                              void* stream) {
  return guarded([&] {
    if (n_parts < 1 || k < 1 || k > 32) fail(KMHG_EINVAL, "bad merge arguments");
    if (!n_kmers || !d_labels || ((opt & KMHG_OPT_POS) && (!n_pos_rows || !d_pos)) ||
        ((opt & KMHG_OPT_PAIRS) && (!n_pair_rows || !d_pairs)) ||
        ((opt & KMHG_OPT_KMER) && !d_kmers) ||
        ((opt & (KMHG_OPT_POS | KMHG_OPT_PAIRS | KMHG_OPT_COUNT)) && !d_counts))
      fail(KMHG_EINVAL, "null argument");
    merge_part_positions(n_parts, opt, k, n_kmers, n_pos_rows, n_pair_rows, d_labels, d_counts,
                         d_kmers, d_pos, d_pairs, d_out_kmers, d_out_pos, d_out_pairs,
                         d_out_counts, (hipStream_t)stream);
  });
}

int kmhg_seq_pack(const void* d_seq, int64_t L, uint32_t* d_code, uint16_t* d_nbit,
                  void* stream) {
  return guarded([&] {
    if (L < 0) fail(KMHG_EINVAL, "bad sequence length");
    if (!L) return;
    if (!d_seq || !d_code || !d_nbit) fail(KMHG_EINVAL, "null argument");
    hipStream_t s = (hipStream_t)stream;
    LAUNCH("k_seq_pack", s, launch_seq_pack(static_cast<const uint8_t*>(d_seq), L, d_code,
                                            d_nbit, s));
    HIPC(hipGetLastError());
  });
}

int kmhg_seq_unpack(const uint32_t* d_code, const uint16_t* d_nbit, int64_t word0, int64_t a,
                    int64_t b, void* d_seq, void* stream) {
  return guarded([&] {
    if (a < 0 || b < a || word0 < 0 || word0 > a / 16) fail(KMHG_EINVAL, "bad unpack range");
    if (b == a) return;
    if (!d_code || !d_nbit || !d_seq) fail(KMHG_EINVAL, "null argument");
    hipStream_t s = (hipStream_t)stream;
    LAUNCH("k_seq_unpack", s, launch_seq_unpack(d_code, d_nbit, (uint64_t)word0, a, b,
                                                static_cast<uint8_t*>(d_seq), s));
    HIPC(hipGetLastError());
  });
}

int kmhg_rows_runs(const void* d_rows, int64_t n_rows, void* d_runs, int64_t cap_runs,
                   int64_t* n_runs, void* stream) {
  return guarded([&] {
    if (n_rows < 0 || n_rows > INT32_MAX || !n_runs) fail(KMHG_EINVAL, "bad run arguments");
    *n_runs = 0;
    if (!n_rows) return;
    if (!d_rows) fail(KMHG_EINVAL, "null argument");
    hipStream_t s = (hipStream_t)stream;
    ReleaseGroup rg(s);
    const uint64_t nt = ((uint64_t)n_rows + TILE - 1) / TILE;
    DBuf<uint64_t> tiles(nt + scan_u64_scratch(nt), s);
    PinnedRec hrec = PinnedPool::get().take();
    GiveBack give_back{hrec, s};
    const int2* rows = reinterpret_cast<const int2*>(d_rows);
    const uint64_t n = count_runs(rows, (uint64_t)n_rows, tiles.p, &hrec.meta->n_kmers, s);
    *n_runs = (int64_t)n;
    if (d_runs && (int64_t)n <= cap_runs)
      LAUNCH("k_runs_emit", s, launch_runs_emit(rows, (uint64_t)n_rows, tiles.p,
                                                static_cast<int32_t*>(d_runs), s));
    HIPC(hipGetLastError());
  });
}

int kmhg_rows_to_host(const void* d_rows, int64_t n_rows, int32_t* rows, void* stream) {
  return guarded([&] {
    if (n_rows < 0) fail(KMHG_EINVAL, "bad row count");
    if (!n_rows) return;
    if (!d_rows || !rows) fail(KMHG_EINVAL, "null argument");
    rows_to_host(static_cast<const int2*>(d_rows), (uint64_t)n_rows, rows, (hipStream_t)stream);
  });
}

int kmhg_runs_expand(const void* d_runs, int64_t n_runs, int64_t n_rows, void* d_rows,
                     void* stream) {
  return guarded([&] {
    if (n_rows < 0 || n_rows > INT32_MAX || n_runs < 0 || n_runs > n_rows || (n_rows && !n_runs))
      fail(KMHG_EINVAL, "bad run arguments");
    if (!n_rows) return;
    if (!d_runs || !d_rows) fail(KMHG_EINVAL, "null argument");
    hipStream_t s = (hipStream_t)stream;
    ReleaseGroup rg(s);
    DBuf<uint32_t> cover(((uint64_t)n_rows + TILE - 1) / TILE, s);
    LAUNCH("k_runs_expand", s,
           launch_runs_expand(static_cast<const int32_t*>(d_runs), (uint64_t)n_runs,
                              (uint64_t)n_rows, cover.p, static_cast<int2*>(d_rows), s));
    HIPC(hipGetLastError());
  });
}

int kmhg_query_fill(kmhg_query* q, int32_t* rows) {
  return guarded([&] {
    if (!q) fail(KMHG_EINVAL, "null query");
    if (q->n_runs >= 0) fail(KMHG_EINVAL, "the query holds runs (kmhg_query_runs_device)");
    if (!q->H) return;
    if (!rows) fail(KMHG_EINVAL, "null output");
    if (!q->parts.empty() && !q->gathered) {   // every part straight into its rows, in parallel
      std::vector<int> each(q->parts.size());
      std::iota(each.begin(), each.end(), 0);
      const Error bad = for_parts(each, [&](int i) {
        kmhg_query* p = q->parts[i];
        if (!p->H) return;
        DeviceGuard g(p->device);
        rows_to_host(p->rows.p, (uint64_t)p->H, rows + 2 * q->part_off[i], lib_stream());
      });
      if (bad.code != KMHG_OK) fail(bad.code, bad.msg);
      return;
    }
    DeviceGuard g(q->device);
    hipStream_t s = lib_stream();
    rows_to_host(q->rows.p, (uint64_t)q->H, rows, s);
  });
}

int kmhg_query_rows_device(kmhg_query* q, const int32_t** d_rows) {
  return guarded([&] {
    if (!q || !d_rows) fail(KMHG_EINVAL, "null argument");
    if (q->n_runs >= 0) fail(KMHG_EINVAL, "the query holds runs (kmhg_query_runs_device)");
    gather_parts(q);
    *d_rows = reinterpret_cast<const int32_t*>(q->rows.p);
  });
}

int kmhg_query_copy_device(kmhg_query* q, void* d_dst, void* stream) {
  return guarded([&] {
    if (!q) fail(KMHG_EINVAL, "null query");
    if (q->n_runs >= 0) fail(KMHG_EINVAL, "the query holds runs (kmhg_query_runs_device)");
    if (!q->H) return;
    if (!d_dst) fail(KMHG_EINVAL, "null output");
    DeviceGuard g(q->device);
    hipStream_t s = (hipStream_t)stream;
    if (!q->parts.empty() && !q->gathered) {   // peer copies of the (finished) parts
      for (size_t i = 0; i < q->parts.size(); ++i)
        if (q->parts[i]->H)
          HIPC(hipMemcpyPeerAsync(static_cast<int2*>(d_dst) + q->part_off[i], q->device,
                                  q->parts[i]->rows.p, q->parts[i]->device,
                                  (size_t)q->parts[i]->H * 8, s));
      return;
    }
    if (s != q->stream) {   // order after the emit kernel queued on q->stream
      hipEvent_t ev;
      HIPC(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      HIPC(hipEventRecord(ev, q->stream));
      HIPC(hipStreamWaitEvent(s, ev, 0));
      HIPC(hipEventDestroy(ev));
    }
    HIPC(hipMemcpyAsync(d_dst, q->rows.p, (size_t)q->H * 8, hipMemcpyDeviceToDevice, s));
  });
}

int kmhg_query_free(kmhg_query* q) {
  return guarded([&] { free_query(q); });
}

// ---------------------------------------------------------------------------- reads.kmer.pos
extern "C++" {
namespace {

ReadsCall checked(const ReadsCall& c) {
  if (c.code != KMHG_OK) fail(c.code, c.text);
  return c;
}

// What a batched read query refuses of the index and of the call, before anything is launched.
ReadsCall reads_checked(const kmhg_index* idx, int64_t n_bases, int64_t n_reads, int k,
                        int strands) {
  if (idx->canonical) fail(KMHG_EINVAL, "External pointer has incorrect tag");
  if (idx->is_part) fail(KMHG_EINVAL, "a part index must be assembled before it is queried");
  return checked(reads_call(n_bases, n_reads, k, strands, idx->sources, idx->k, idx->sampling))
      .with_max_occ(idx->max_occ.load(std::memory_order_relaxed));
}

// The batch on the index's device (kmhg_readsq.hip): the offsets' check, probe, mask, scan and
// emit queued on `s`, one wait for the row total and the check's flag, and the rows emitted again
// into an exact buffer where the guess was short.
kmhg_rquery* reads_query_device(kmhg_index* idx, const uint8_t* d_seq, const int64_t* d_off,
                                const ReadsCall& c, hipStream_t s) {
  ReleaseGroup rg(s);
  finish_build(idx);
  auto q = std::make_unique<kmhg_rquery>();
  q->device = idx->device;
  q->stream = s;
  q->n_reads = c.n_reads;
  q->k = c.k;
  idx->stream = s;
  PinnedRec hrec = PinnedPool::get().take();
  GiveBack give_back{hrec, s};
  uint64_t* total = &hrec.meta->n_kmers;
  uint32_t* bad_off = &hrec.meta->n_small;
  LAUNCH("k_rq_check", s, launch_rq_check(d_off, c.n_reads, c.n_bases, bad_off, s));
  const int64_t V = rq_virtual(c.n_bases, c.ns);
  if (V == 0) {
    HIPC(hipStreamSynchronize(s));
    if (__atomic_load_n(bad_off, __ATOMIC_ACQUIRE)) fail(KMHG_EINVAL, RQ_OFF_TEXT);
    return q.release();
  }
  const uint32_t nt = tiles_for((uint64_t)V);
  uint64_t cap = rq_rows_guess(V);
  q->rows.reset(RQ_ROW_INTS * cap);
  DBuf<uint32_t> qrec(V, s);
  DBuf<uint2> qmulti(V, s);
  DBuf<uint64_t> tiles((size_t)nt + scan_u64_scratch(nt), s);
  LAUNCH("k_rq_probe", s,
         launch_rq_probe(d_seq, c.n_bases, d_off, c.n_reads, c.k, c.ns, c.rev_only, idx->table.p,
                         idx->geom, qrec.p, qmulti.p, tiles.p, s));
  if (c.max_occ)
    LAUNCH("k_qrec_mask", s,
           launch_qrec_mask(qrec.p, qmulti.p, V, (uint32_t)c.max_occ, tiles.p, s));
  LAUNCH("k_scan_tiles_u64", s, launch_scan_u64(tiles.p, nt, total, tiles.p + nt, s));
  LAUNCH("k_rq_emit", s,
         launch_rq_emit(qrec.p, qmulti.p, d_off, c.n_reads, c.n_bases, c.k, c.ns, c.rev_only,
                        idx->positions.p, tiles.p, q->rows.p, cap, s));
  HIPC(hipStreamSynchronize(s));
  if (__atomic_load_n(bad_off, __ATOMIC_ACQUIRE)) fail(KMHG_EINVAL, RQ_OFF_TEXT);
  const uint64_t H = __atomic_load_n(total, __ATOMIC_ACQUIRE);
  q->H = (int64_t)H;
  if (!needs_exact_redo(H, cap)) {
    rg.synced = true;                              // nothing queued behind the synchronize
    return q.release();
  }
  q->rows.bind(s);
  q->rows.reset(RQ_ROW_INTS * H);
  LAUNCH("k_rq_emit", s,
         launch_rq_emit(qrec.p, qmulti.p, d_off, c.n_reads, c.n_bases, c.k, c.ns, c.rev_only,
                        idx->positions.p, tiles.p, q->rows.p, H, s));
  HIPC(hipStreamSynchronize(s));
  return q.release();
}

// Host reads: the offsets are looked at before anything is copied.
void reads_query_host(kmhg_index* idx, const uint8_t* seq, int64_t n_bases, const int64_t* off,
                      int64_t n_reads, int k, int strands, kmhg_rquery** q, int64_t* n_rows) {
  if (!idx || !q || !off || (n_bases > 0 && !seq)) fail(KMHG_EINVAL, "null argument");
  const ReadsCall c = reads_checked(idx, n_bases, n_reads, k, strands);
  checked(reads_off_refusal(off, n_reads, n_bases));
  DeviceGuard g(idx->device);
  hipStream_t s = lib_stream();
  DBuf<uint8_t> d_seq((size_t)n_bases + 16, s);
  DBuf<int64_t> d_off((size_t)n_reads + 1, s);
  h2d_host(d_seq.p, seq, (size_t)n_bases, s);
  h2d_host(d_off.p, off, ((size_t)n_reads + 1) * sizeof(int64_t), s);
  *q = reads_query_device(idx, d_seq.p, d_off.p, c, s);
  if (n_rows) *n_rows = (*q)->H;
}

// reads.kmer.vote of n_rows rows on the current device into d_votes; waits for `s`.
void rows_votes_device(const int32_t* d_rows, int64_t n_rows, int64_t n_reads, int k, int64_t band,
                       int32_t* d_votes, hipStream_t s) {
  checked(vote_refusal(n_rows, n_reads, k, band));
  if (!n_reads && n_rows)
    fail(KMHG_EINVAL, "rows must have a read in 1 .. n_reads and a strand of +1 or -1");
  if (!n_reads) return;
  if (!d_votes || (n_rows && !d_rows)) fail(KMHG_EINVAL, "null argument");
  ReleaseGroup rg(s);
  const uint64_t n = (uint64_t)n_rows;
  size_t tb = 0;
  if (n) HIPC(vote_temp_bytes(n, &tb));
  DBuf<uint8_t> temp(std::max<size_t>(tb, 16), s);
  DBuf<uint64_t> keys(3 * n + (size_t)n_reads, s);     // keys, sorted keys, cells; then best
  DBuf<uint32_t> u32s(n + 1 + 2 * (size_t)n_reads, s); // votes, n_cells; then second, total
  uint64_t* cells = keys.p + 2 * n;
  uint64_t* best = keys.p + 3 * n;
  uint32_t* votes = u32s.p;
  uint32_t* n_cells = u32s.p + n;
  uint32_t* second = u32s.p + n + 1;
  uint32_t* total = second + n_reads;
  PinnedRec hrec = PinnedPool::get().take();
  GiveBack give_back{hrec, s};
  uint32_t* bad = &hrec.meta->n_small;
  hipError_t err = hipSuccess;
  LAUNCH("k_votes", s,
         err = launch_votes(d_rows, n, n_reads, k, band, keys.p, cells, votes, n_cells, temp.p, tb,
                            best, second, total, d_votes, bad, s));
  HIPC(err);
  HIPC(hipStreamSynchronize(s));
  rg.synced = true;
  if (__atomic_load_n(bad, __ATOMIC_ACQUIRE))
    fail(KMHG_EINVAL, "rows must have a read in 1 .. n_reads and a strand of +1 or -1");
}

}  // namespace
}  // extern "C++"

int kmhg_reads_query_run_device(kmhg_index* idx, const void* d_seq, int64_t n_bases,
                                const int64_t* d_off, int64_t n_reads, int k, int strands,
                                void* stream, kmhg_rquery** q, int64_t* n_rows) {
  return guarded([&] {
    if (!idx || !q || !d_off || (n_bases > 0 && !d_seq)) fail(KMHG_EINVAL, "null argument");
    const ReadsCall c = reads_checked(idx, n_bases, n_reads, k, strands);
    DeviceGuard g(idx->device);
    *q = reads_query_device(idx, static_cast<const uint8_t*>(d_seq), d_off, c, (hipStream_t)stream);
    if (n_rows) *n_rows = (*q)->H;
  });
}

int kmhg_reads_query_run_packed(kmhg_index* idx, const uint8_t* seq, int64_t n_bases,
                                const int64_t* off, int64_t n_reads, int k, int strands,
                                kmhg_rquery** q, int64_t* n_rows) {
  return guarded([&] { reads_query_host(idx, seq, n_bases, off, n_reads, k, strands, q, n_rows); });
}

int kmhg_reads_query_run(kmhg_index* idx, const kmhg_reads* r, int k, int strands, kmhg_rquery** q,
                         int64_t* n_rows) {
  return guarded([&] {
    if (!r) fail(KMHG_EINVAL, "null argument");
    reads_query_host(idx, r->r.seq.data(), (int64_t)r->r.seq.size(), r->r.off.data(),
                     (int64_t)r->r.n(), k, strands, q, n_rows);
  });
}

int kmhg_rquery_rows_device(kmhg_rquery* q, const int32_t** d_rows, int64_t* n_rows) {
  return guarded([&] {
    if (!q || !d_rows) fail(KMHG_EINVAL, "null argument");
    *d_rows = q->rows.p;
    if (n_rows) *n_rows = q->H;
  });
}

int kmhg_rquery_copy_device(kmhg_rquery* q, void* d_dst, void* stream) {
  return guarded([&] {
    if (!q) fail(KMHG_EINVAL, "null query");
    if (!q->H) return;
    if (!d_dst) fail(KMHG_EINVAL, "null output");
    DeviceGuard g(q->device);
    HIPC(hipMemcpyAsync(d_dst, q->rows.p, rq_rows_bytes((uint64_t)q->H), hipMemcpyDeviceToDevice,
                        (hipStream_t)stream));
  });
}

int kmhg_rquery_fill(kmhg_rquery* q, int32_t* rows) {
  return guarded([&] {
    if (!q) fail(KMHG_EINVAL, "null query");
    checked(rq_fill_refusal(q->H));
    if (!q->H) return;
    if (!rows) fail(KMHG_EINVAL, "null output");
    DeviceGuard g(q->device);
    hipStream_t s = lib_stream();
    d2h_host(rows, q->rows.p, rq_rows_bytes((uint64_t)q->H), s);
    HIPC(hipStreamSynchronize(s));
  });
}

int kmhg_rquery_free(kmhg_rquery* q) {
  return guarded([&] {
    if (!q) return;
    DeviceGuard g(q->device);
    HIPC(hipStreamSynchronize(q->stream));
    q->rows.ordered = false;               // its stream is idle: straight back to the pool
    delete q;
  });
}

int kmhg_rrows_votes(const void* d_rows, int64_t n_rows, int64_t n_reads, int k, int64_t band,
                     void* d_votes, void* stream) {
  return guarded([&] {
    rows_votes_device(static_cast<const int32_t*>(d_rows), n_rows, n_reads, k, band,
                      static_cast<int32_t*>(d_votes), (hipStream_t)stream);
  });
}

int kmhg_rquery_votes_device(kmhg_rquery* q, int64_t band, void* d_votes, void* stream) {
  return guarded([&] {
    if (!q) fail(KMHG_EINVAL, "null query");
    DeviceGuard g(q->device);
    rows_votes_device(q->rows.p, q->H, q->n_reads, q->k, band, static_cast<int32_t*>(d_votes),
                      (hipStream_t)stream);
  });
}

int kmhg_rquery_votes(kmhg_rquery* q, int64_t band, int32_t* votes) {
  return guarded([&] {
    if (!q) fail(KMHG_EINVAL, "null query");
    checked(vote_refusal(q->H, q->n_reads, q->k, band));
    if (!q->n_reads) return;
    if (!votes) fail(KMHG_EINVAL, "null output");
    DeviceGuard g(q->device);
    hipStream_t s = lib_stream();
    DBuf<int32_t> d((size_t)VOTE_COLS * (size_t)q->n_reads, s);
    rows_votes_device(q->rows.p, q->H, q->n_reads, q->k, band, d.p, s);
    d2h_host(votes, d.p, d.bytes(), s);
    HIPC(hipStreamSynchronize(s));
  });
}

// ---------------------------------------------------------------------------- seq.kmer.segs
namespace {

// The front half of the segment pass, which seq.kmer.segs and seq.kmer.blocks share: segment m of
// the (diagonal, i) order has the pairing keys skey()[m] (its first row) and ekey()[m] (its last)
// and rank()[m], its first row's rank among all starts in row order.
struct SegPairs {
  uint64_t S = 0;
  DBuf<uint64_t> keys;                  // start, end keys; both sorted
  DBuf<uint32_t> ranks;
  const uint64_t* skey() const { return keys.p + 2 * S; }
  const uint64_t* ekey() const { return keys.p + 3 * S; }
  const uint32_t* rank() const { return ranks.p + S; }
  // where an emit kernel writes the keys (ranks: ranks.p) before sort_seg_pairs
  uint64_t* skey_in() { return keys.p; }
  uint64_t* ekey_in() { return keys.p + S; }
  void alloc(uint64_t n_segs, hipStream_t s) {
    S = n_segs;
    keys.reset(4 * S);
    keys.bind(s);
    ranks.reset(2 * S);
    ranks.bind(s);
  }
};

// Both key arrays ascending, the starts' ranks carried (kmhg_segs.hip).
void sort_seg_pairs(SegPairs& sp, hipStream_t s) {
  const uint64_t S = sp.S;
  size_t tb = 0;
  HIPC(segs_sort_temp_bytes(S, &tb));
  DBuf<uint8_t> temp(std::max<size_t>(tb, 16), s);
  hipError_t sort_err = hipSuccess;
  LAUNCH("k_segs_sort", s,
         sort_err = launch_segs_sort(sp.skey_in(), sp.ranks.p, sp.ekey_in(), S, sp.keys.p + 2 * S,
                                     sp.ranks.p + S, sp.keys.p + 3 * S, temp.p, tb, s));
  HIPC(sort_err);
}

// What the row-free routes (segs_pairs_from_records, raster_device) refuse of an index before
// they probe it, query_device's checks; then its pending build is finished.  positions_only: the
// refusal of an index with sources (a counts index), or null where the route takes one.
void records_index(kmhg_index* idx, const QueryCall& c, hipStream_t s, const char* positions_only) {
  if (idx->canonical) fail(KMHG_EINVAL, "External pointer has incorrect tag");
  if (idx->is_part != c.part)
    fail(KMHG_EINVAL, idx->is_part ? "a part index must be assembled before it is queried"
                                   : "not a part of an owner-computes build");
  if (positions_only && idx->sources) fail(KMHG_EINVAL, positions_only);
  finish_build(idx);
  idx->stream = s;
}

// The per-window records of a probed query (put_qrec) and the probe's per-tile hit totals.
struct QueryRecords {
  DBuf<uint32_t> qrec;
  DBuf<uint2> qmulti;
  DBuf<uint64_t> tiles;
};

// query_device's probe of the c.w1 - c.w0 > 0 windows, without the emit list, and the scan of
// the tile totals: *total (pinned) <- the hit total once `s` has been waited for.
void probe_records(kmhg_index* idx, const uint8_t* d_seq, const QueryCall& c, uint64_t* total,
                   hipStream_t s, QueryRecords& r) {
  const int64_t Nw = c.w1 - c.w0;
  const int kq = c.k;
  const bool aligned = (reinterpret_cast<uintptr_t>(d_seq) & 15) == 0;
  const uint32_t nt = tiles_for(Nw);
  const char* de = test_build_knob("KMHG_QUERY_DIAG");
  const bool diag = diag_eligible(kq, idx->k, idx->sources, idx->L - idx->k + 1, idx->U,
                                  idx->dcodes.p != nullptr, !(de && de[0] == '0'), idx->sampling) &&
                    ensure_diag(idx, s);
  r.qrec.reset(Nw);
  r.qrec.bind(s);
  r.qmulti.reset(Nw);
  r.qmulti.bind(s);
  r.tiles.reset((size_t)nt + scan_u64_scratch(nt));
  r.tiles.bind(s);
  LAUNCH("k_query_probe", s,
         launch_query_probe(d_seq, c.L, kq, idx->table.p, idx->geom, r.qrec.p, r.qmulti.p, c.w0, c.w1,
                            aligned, r.tiles.p, s,
                            diag ? idx->diag_view() : DiagIdx{nullptr, nullptr, 0},
                            diag && tags_on() ? idx->ptag.p : nullptr, nullptr, c.rc));
  mask_records(c, d_seq, r.qrec.p, r.qmulti.p, r.tiles.p, s);
  LAUNCH("k_scan_tiles_u64", s, launch_scan_u64(r.tiles.p, nt, total, r.tiles.p + nt, s));
}

// Classifies and counts the starts and ends of n ascending rows, waits for `s` once (the number
// of segments sizes the sort) and answers the two row faults; then, with `pair`, emits the
// pairing keys and sorts them (kmhg_segs.hip).  hm: the caller's pinned record (n_kmers: the scan
// totals; n_small / n_large: the faults).
void segs_sorted_pairs(const int2* rows, uint64_t n, bool pair, BuildMeta* hm, hipStream_t s,
                       SegPairs& sp) {
  const uint64_t nt = (n + TILE - 1) / TILE;
  DBuf<uint64_t> tiles(nt + scan_u64_scratch(nt), s);
  DBuf<uint64_t> masks(2 * nt * (TILE / 64), s);
  uint64_t* smask = masks.p;
  uint64_t* emask = masks.p + nt * (TILE / 64);
  __atomic_store_n(&hm->n_small, 0u, __ATOMIC_RELEASE);
  __atomic_store_n(&hm->n_large, 0u, __ATOMIC_RELEASE);
  LAUNCH("k_segs_classify", s, launch_segs_classify(rows, n, smask, emask, tiles.p, &hm->n_small,
                                                    &hm->n_large, s));
  LAUNCH("k_scan_tiles_u64", s, launch_scan_u64(tiles.p, nt, &hm->n_kmers, tiles.p + nt, s));
  HIPC(hipStreamSynchronize(s));
  if (__atomic_load_n(&hm->n_large, __ATOMIC_ACQUIRE)) fail(KMHG_EINVAL, "rows must have i, j >= 1");
  if (__atomic_load_n(&hm->n_small, __ATOMIC_ACQUIRE))
    fail(KMHG_EINVAL, "rows are not in ascending (i, j) order");
  const uint64_t both = __atomic_load_n(&hm->n_kmers, __ATOMIC_ACQUIRE);
  const uint64_t S = both & 0xFFFFFFFFull;
  // on every diagonal starts and ends alternate, so there are as many of each
  if (!S || (both >> 32) != S) fail(KMHG_EDEVICE, "segment starts and ends do not pair");
  if (!pair) return;
  sp.alloc(S, s);
  LAUNCH("k_segs_emit", s,
         launch_segs_emit(rows, n, smask, emask, tiles.p, sp.skey_in(), sp.ranks.p, sp.ekey_in(), s));
  sort_seg_pairs(sp, s);
}

// The same front half without rows (kmhg_segrec.hip): probes the query as raster_device does,
// counts the starts and ends of every tile from the window records, waits for `s` once (the hit
// total, and the number of segments, which sizes the sort), then emits the pairing keys from the
// records again and sorts them.  Returns the hit total H, which may exceed 2^31 - 1; H = 0 leaves
// sp empty.  Scratch is O(Nw + Nw / TILE + S): nothing grows with H.  hm: the caller's pinned
// record (n_kmers: H; n_positions / n_pairs: the starts and the ends).
uint64_t segs_pairs_from_records(kmhg_index* idx, const uint8_t* d_seq, const QueryCall& c,
                                 BuildMeta* hm, hipStream_t s, SegPairs& sp) {
  const int64_t Nw = c.w1 - c.w0;
  if (Nw <= 0) return 0;
  const uint32_t nt = tiles_for(Nw);
  QueryRecords r;
  probe_records(idx, d_seq, c, &hm->n_kmers, s, r);
  const size_t per = (size_t)nt + scan_u64_scratch(nt);
  DBuf<uint64_t> cnt(2 * per, s);                   // per tile: starts, ends (each with its scan's)
  DBuf<uint32_t> wstarts(Nw, s);                    // per window: starts
  uint64_t *ts = cnt.p, *te = cnt.p + per;
  LAUNCH("k_segrec_count", s,
         launch_segrec_count(r.qrec.p, r.qmulti.p, Nw, idx->positions.p, ts, te, wstarts.p, s));
  LAUNCH("k_scan_tiles_u64", s, launch_scan_u64(ts, nt, &hm->n_positions, ts + nt, s));
  LAUNCH("k_scan_tiles_u64", s, launch_scan_u64(te, nt, &hm->n_pairs, te + nt, s));
  HIPC(hipStreamSynchronize(s));
  const uint64_t H = __atomic_load_n(&hm->n_kmers, __ATOMIC_ACQUIRE);
  if (!H) return 0;
  const uint64_t S = __atomic_load_n(&hm->n_positions, __ATOMIC_ACQUIRE);
  const SegrecRefusal rf = segrec_check_totals(S, __atomic_load_n(&hm->n_pairs, __ATOMIC_ACQUIRE));
  if (rf.code != KMHG_OK) fail(rf.code, rf.text);
  sp.alloc(S, s);
  LAUNCH("k_segrec_emit", s,
         launch_segrec_emit(r.qrec.p, r.qmulti.p, Nw, c.w0, c.k, idx->positions.p, wstarts.p, ts, te,
                            S, sp.skey_in(), sp.ranks.p, sp.ekey_in(), s));
  sort_seg_pairs(sp, s);
  return H;
}

// The back half of the segment pass: {i, j, len} of the sorted pairs at their starts' ranks, the
// segments with len >= min_len (<= INT32_MAX) kept, into g.  Waits for `s` (min_len > 1: the
// number kept sizes the result) and once more at the end.  hm: the caller's pinned record.
void pairs_segments(const SegPairs& sp, int64_t min_len, BuildMeta* hm, hipStream_t s,
                    kmhg_segs* g) {
  const uint64_t S = sp.S;
  if (min_len == 1) {
    g->segs.reset(3 * S);
    LAUNCH("k_segs_pair", s, launch_segs_pair(sp.skey(), sp.rank(), sp.ekey(), S, g->segs.p, s));
    g->S = (int64_t)S;
  } else {
    DBuf<int32_t> all(3 * S, s);
    LAUNCH("k_segs_pair", s, launch_segs_pair(sp.skey(), sp.rank(), sp.ekey(), S, all.p, s));
    const uint64_t nts = (S + TILE - 1) / TILE;
    DBuf<uint64_t> ftiles(nts + scan_u64_scratch(nts), s);
    LAUNCH("k_segs_filter", s, launch_segs_filter_count(all.p, S, (int32_t)min_len, ftiles.p, s));
    LAUNCH("k_scan_tiles_u64", s,
           launch_scan_u64(ftiles.p, nts, &hm->n_positions, ftiles.p + nts, s));
    HIPC(hipStreamSynchronize(s));
    const uint64_t K = __atomic_load_n(&hm->n_positions, __ATOMIC_ACQUIRE);
    g->segs.reset(3 * K);
    if (K)
      LAUNCH("k_segs_filter", s, launch_segs_filter_emit(all.p, S, (int32_t)min_len, ftiles.p,
                                                         g->segs.p, s));
    g->S = (int64_t)K;
  }
  HIPC(hipStreamSynchronize(s));
}

// The maximal diagonal segments of n_rows ascending rows on the current device (kmhg_segs.hip;
// include/kmhgpu.h has the definition).  Waits for `s` twice (the number of segments sizes the
// sort; min_len > 1: the number kept sizes the result) and once more at the end.
kmhg_segs* rows_segments(const int2* rows, int64_t n_rows, int64_t min_len, hipStream_t s) {
  auto g = std::make_unique<kmhg_segs>();
  if (!n_rows) return g.release();      // (no device call: an empty result is host-only)
  HIPC(hipGetDevice(&g->device));
  g->stream = s;
  ReleaseGroup rg(s);
  PinnedRec hrec = PinnedPool::get().take();
  GiveBack give_back{hrec, s};
  BuildMeta* hm = hrec.meta;
  SegPairs sp;
  segs_sorted_pairs(rows, (uint64_t)n_rows, min_len <= INT32_MAX, hm, s, sp);
  if (min_len > INT32_MAX) return g.release();            // no segment has that many rows
  pairs_segments(sp, min_len, hm, s, g.get());
  rg.synced = true;
  return g.release();
}

// The back half of the block pass: the sorted pairs filtered by min_len, then heads / mark /
// place / order, into g (min_len, min_hits <= INT32_MAX).  Waits for `s` where a count sizes an
// allocation -- min_len > 1: the number of segments kept, and the number of blocks (the result)
// -- and once more at the end: `s` is idle when it returns.  hm: the caller's pinned record.
void pairs_blocks(const SegPairs& sp, int64_t min_len, int64_t max_gap, int64_t min_hits,
                  BuildMeta* hm, hipStream_t s, kmhg_blocks* g) {
  const uint64_t S = sp.S;
  const uint32_t gap_limit = blk_gap_limit(max_gap);
  const uint64_t *skey = sp.skey(), *ekey = sp.ekey();
  const uint32_t* rank = sp.rank();
  uint64_t K = S;
  DBuf<uint64_t> fkeys;
  DBuf<uint32_t> franks;
  if (min_len > 1) {
    const uint64_t nts = (S + TILE - 1) / TILE;
    DBuf<uint64_t> ftiles(nts + scan_u64_scratch(nts), s);
    LAUNCH("k_blocks_filter", s,
           launch_blocks_filter_count(skey, ekey, S, (int32_t)min_len, ftiles.p, s));
    LAUNCH("k_scan_tiles_u64", s,
           launch_scan_u64(ftiles.p, nts, &hm->n_positions, ftiles.p + nts, s));
    HIPC(hipStreamSynchronize(s));
    K = __atomic_load_n(&hm->n_positions, __ATOMIC_ACQUIRE);
    if (!K) return;
    fkeys.reset(2 * K);
    fkeys.bind(s);
    franks.reset(K);
    franks.bind(s);
    LAUNCH("k_blocks_filter", s,
           launch_blocks_filter_emit(skey, ekey, rank, S, (int32_t)min_len, ftiles.p, fkeys.p,
                                     fkeys.p + K, franks.p, s));
    skey = fkeys.p;
    ekey = fkeys.p + K;
    rank = franks.p;
  }
  const uint64_t ntk = (K + TILE - 1) / TILE, nts = (S + TILE - 1) / TILE;
  DBuf<uint64_t> htiles(ntk + 1 + scan_u64_scratch(ntk), s);   // [ntk]: the scan's total
  DBuf<uint64_t> bkeys(2 * K, s);                              // per block id: start, end key
  DBuf<uint32_t> bnum(3 * K, s);                               // rank, len prefix before / after
  DBuf<uint32_t> slot(S, s);
  DBuf<uint64_t> otiles(nts + scan_u64_scratch(nts), s);
  LAUNCH("k_blocks_heads", s, launch_blocks_heads(skey, ekey, K, gap_limit, htiles.p, s));
  LAUNCH("k_scan_tiles_u64", s,
         launch_scan_u64(htiles.p, ntk, htiles.p + ntk, htiles.p + ntk + 1, s));
  LAUNCH("k_blocks_mark", s,
         launch_blocks_mark(skey, ekey, rank, K, gap_limit, htiles.p, bkeys.p, bkeys.p + K,
                            bnum.p, bnum.p + K, bnum.p + 2 * K, s));
  HIPC(hipMemsetAsync(slot.p, 0, (size_t)S * 4, s));
  LAUNCH("k_blocks_place", s,
         launch_blocks_place(htiles.p + ntk, K, bnum.p, bnum.p + K, bnum.p + 2 * K,
                             (uint32_t)min_hits, slot.p, s));
  LAUNCH("k_blocks_order", s, launch_blocks_order_count(slot.p, S, otiles.p, s));
  LAUNCH("k_scan_tiles_u64", s, launch_scan_u64(otiles.p, nts, &hm->n_pairs, otiles.p + nts, s));
  HIPC(hipStreamSynchronize(s));
  const uint64_t B = __atomic_load_n(&hm->n_pairs, __ATOMIC_ACQUIRE);
  if (B) {
    g->blocks.reset(4 * B);
    LAUNCH("k_blocks_order", s,
           launch_blocks_order_emit(slot.p, S, otiles.p, bkeys.p, bkeys.p + K, bnum.p + K,
                                    bnum.p + 2 * K, g->blocks.p, s));
    g->B = (int64_t)B;
    HIPC(hipStreamSynchronize(s));
  }
}

// The blocks of n_rows ascending rows on the current device (kmhg_blocks.hip; include/kmhgpu.h
// has the definition): the segment pass's sorted keys, filtered by min_len, then heads / mark /
// place / order.  Waits for `s` where a count sizes an allocation -- the number of segments (the
// sort), min_len > 1: the number kept, and the number of blocks (the result) -- and once more at
// the end.  The number of blocks before min_hits stays on the device.
kmhg_blocks* rows_blocks(const int2* rows, int64_t n_rows, int64_t min_len, int64_t max_gap,
                         int64_t min_hits, hipStream_t s) {
  auto g = std::make_unique<kmhg_blocks>();
  if (!n_rows) return g.release();      // (no device call: an empty result is host-only)
  HIPC(hipGetDevice(&g->device));
  g->stream = s;
  ReleaseGroup rg(s);
  PinnedRec hrec = PinnedPool::get().take();
  GiveBack give_back{hrec, s};
  BuildMeta* hm = hrec.meta;            // n_positions: segments kept; n_pairs: blocks
  // no segment has 2^31 rows and no block 2^31 hits
  const bool any = min_len <= INT32_MAX && min_hits <= INT32_MAX;
  SegPairs sp;
  segs_sorted_pairs(rows, (uint64_t)n_rows, any, hm, s, sp);
  if (!any) return g.release();
  pairs_blocks(sp, min_len, max_gap, min_hits, hm, s, g.get());
  rg.synced = true;
  return g.release();
}

void check_segs_args(int64_t min_len, kmhg_segs** out) {
  if (!out) fail(KMHG_EINVAL, "null argument");
  if (min_len < 1) fail(KMHG_EINVAL, "min_len must be a positive integer");
}

// seq.kmer.segs without rows: the records front half, then the same back half.  *H <- the hit
// total; H = 0 gives an empty handle.
kmhg_segs* records_segments(kmhg_index* idx, const uint8_t* d_seq, const QueryCall& c,
                            int64_t min_len, hipStream_t s, uint64_t* H) {
  auto g = std::make_unique<kmhg_segs>();
  ReleaseGroup rg(s);
  records_index(idx, c, s, "segments need a position index");
  PinnedRec hrec = PinnedPool::get().take();
  GiveBack give_back{hrec, s};
  BuildMeta* hm = hrec.meta;
  SegPairs sp;
  *H = segs_pairs_from_records(idx, d_seq, c, hm, s, sp);
  if (!*H || min_len > INT32_MAX) return g.release();     // no segment has that many rows
  HIPC(hipGetDevice(&g->device));
  g->stream = s;
  pairs_segments(sp, min_len, hm, s, g.get());
  rg.synced = true;
  return g.release();
}

}  // namespace

int kmhg_rows_segments(const void* d_rows, int64_t n_rows, int64_t min_len, void* stream,
                       kmhg_segs** out, int64_t* n_segs) {
  return guarded([&] {
    check_segs_args(min_len, out);
    if (n_rows < 0 || n_rows > INT32_MAX) fail(KMHG_EINVAL, "bad row count");
    if (n_rows && !d_rows) fail(KMHG_EINVAL, "null argument");
    *out = rows_segments(static_cast<const int2*>(d_rows), n_rows, min_len, (hipStream_t)stream);
    if (n_segs) *n_segs = (*out)->S;
  });
}

int kmhg_query_segments(kmhg_query* q, int64_t min_len, kmhg_segs** out, int64_t* n_segs) {
  return guarded([&] {
    if (!q) fail(KMHG_EINVAL, "null argument");
    check_segs_args(min_len, out);
    if (q->n_runs >= 0) fail(KMHG_EINVAL, "the query holds runs (kmhg_query_runs_device)");
    if (q->H > INT32_MAX) fail(KMHG_EINVAL, "bad row count");
    gather_parts(q);                    // a multi-device query's rows, on its home device
    DeviceGuard g(q->device);
    *out = rows_segments(q->rows.p, q->H, min_len, q->stream);
    if (n_segs) *n_segs = (*out)->S;
  });
}

int kmhg_segments_run_device(kmhg_index* idx, const void* d_seq, size_t L, int k, int rc,
                             int64_t min_len, void* stream, kmhg_segs** out, int64_t* n_segs,
                             int64_t* n_rows) {
  return guarded([&] {
    if (!idx || !d_seq) fail(KMHG_EINVAL, "null argument");
    check_segs_args(min_len, out);
    const QueryCall c = capped(idx, query_call(L, k)).on_rc(rc != 0);
    DeviceGuard g(idx->device);
    uint64_t H = 0;
    *out = records_segments(idx, static_cast<const uint8_t*>(d_seq), c, min_len,
                            (hipStream_t)stream, &H);
    if (n_segs) *n_segs = (*out)->S;
    if (n_rows) *n_rows = (int64_t)H;
  });
}

int kmhg_segments_run(kmhg_index* idx, const char* seq, size_t L, int k, int rc, int64_t min_len,
                      kmhg_segs** out, int64_t* n_segs, int64_t* n_rows) {
  return guarded([&] {
    if (!idx || !seq) fail(KMHG_EINVAL, "null argument");
    check_segs_args(min_len, out);
    if (L < H2D_SCAN_MIN || k < 1 || k > 31 || L >= (size_t)INT32_MAX) {
      L = effective_len(seq, L);             // (as kmhg_query_run)
      check_query_args(L, k);
    }
    DeviceGuard g(idx->device);
    hipStream_t s = lib_stream();
    DBuf<uint8_t> d(L + 16, s);
    L = h2d_cstring(d.p, seq, L, s);
    uint64_t H = 0;
    *out = records_segments(idx, d.p, capped(idx, query_call(L, k)).on_rc(rc != 0), min_len, s, &H);
    if (n_segs) *n_segs = (*out)->S;
    if (n_rows) *n_rows = (int64_t)H;
  });
}

int kmhg_segs_device(kmhg_segs* g, const int32_t** d_segs, int64_t* n_segs) {
  return guarded([&] {
    if (!g || !d_segs) fail(KMHG_EINVAL, "null argument");
    *d_segs = g->S ? g->segs.p : nullptr;
    if (n_segs) *n_segs = g->S;
  });
}

int kmhg_segs_copy_device(kmhg_segs* g, void* d_dst, void* stream) {
  return guarded([&] {
    if (!g) fail(KMHG_EINVAL, "null argument");
    if (!g->S) return;
    if (!d_dst) fail(KMHG_EINVAL, "null output");
    DeviceGuard dg(g->device);
    HIPC(hipMemcpyAsync(d_dst, g->segs.p, (size_t)g->S * 12, hipMemcpyDeviceToDevice,
                        (hipStream_t)stream));
  });
}

int kmhg_segs_fill(kmhg_segs* g, int32_t* segs) {
  return guarded([&] {
    if (!g) fail(KMHG_EINVAL, "null argument");
    if (!g->S) return;
    if (!segs) fail(KMHG_EINVAL, "null output");
    DeviceGuard dg(g->device);
    d2h_host(segs, g->segs.p, (size_t)g->S * 12, lib_stream());
  });
}

int kmhg_segs_free(kmhg_segs* g) {
  return guarded([&] {
    if (!g) return;
    std::unique_ptr<kmhg_segs> own(g);
    if (!g->S) return;
    DeviceGuard dg(g->device);
    // the caller keeps the stream it made the segments on alive until here (as for a query)
    HIPC(hipStreamSynchronize(g->stream));
  });
}

// -------------------------------------------------------------------------- seq.kmer.blocks
namespace {

void check_blocks_args(int64_t min_len, int64_t max_gap, int64_t min_hits, kmhg_blocks** out) {
  if (!out) fail(KMHG_EINVAL, "null argument");
  if (min_len < 1) fail(KMHG_EINVAL, "min_len must be a positive integer");
  if (max_gap < 0) fail(KMHG_EINVAL, "max_gap must not be negative");
  if (min_hits < 1) fail(KMHG_EINVAL, "min_hits must be a positive integer");
}

// seq.kmer.blocks without rows: the records front half, then the same back half.  *H <- the hit
// total; H = 0 gives an empty handle.
kmhg_blocks* records_blocks(kmhg_index* idx, const uint8_t* d_seq, const QueryCall& c,
                            int64_t min_len, int64_t max_gap, int64_t min_hits, hipStream_t s,
                            uint64_t* H) {
  auto g = std::make_unique<kmhg_blocks>();
  ReleaseGroup rg(s);
  records_index(idx, c, s, "blocks need a position index");
  PinnedRec hrec = PinnedPool::get().take();
  GiveBack give_back{hrec, s};
  BuildMeta* hm = hrec.meta;            // n_positions: segments kept; n_pairs: blocks
  SegPairs sp;
  *H = segs_pairs_from_records(idx, d_seq, c, hm, s, sp);
  // no segment has 2^31 rows and no block 2^31 hits
  if (!*H || min_len > INT32_MAX || min_hits > INT32_MAX) return g.release();
  HIPC(hipGetDevice(&g->device));
  g->stream = s;
  pairs_blocks(sp, min_len, max_gap, min_hits, hm, s, g.get());
  rg.synced = true;
  return g.release();
}

}  // namespace

int kmhg_blocks_run_device(kmhg_index* idx, const void* d_seq, size_t L, int k, int rc,
                           int64_t min_len, int64_t max_gap, int64_t min_hits, void* stream,
                           kmhg_blocks** out, int64_t* n_blocks, int64_t* n_rows) {
  return guarded([&] {
    if (!idx || !d_seq) fail(KMHG_EINVAL, "null argument");
    check_blocks_args(min_len, max_gap, min_hits, out);
    const QueryCall c = capped(idx, query_call(L, k)).on_rc(rc != 0);
    DeviceGuard g(idx->device);
    uint64_t H = 0;
    *out = records_blocks(idx, static_cast<const uint8_t*>(d_seq), c, min_len, max_gap, min_hits,
                          (hipStream_t)stream, &H);
    if (n_blocks) *n_blocks = (*out)->B;
    if (n_rows) *n_rows = (int64_t)H;
  });
}

int kmhg_blocks_run(kmhg_index* idx, const char* seq, size_t L, int k, int rc, int64_t min_len,
                    int64_t max_gap, int64_t min_hits, kmhg_blocks** out, int64_t* n_blocks,
                    int64_t* n_rows) {
  return guarded([&] {
    if (!idx || !seq) fail(KMHG_EINVAL, "null argument");
    check_blocks_args(min_len, max_gap, min_hits, out);
    if (L < H2D_SCAN_MIN || k < 1 || k > 31 || L >= (size_t)INT32_MAX) {
      L = effective_len(seq, L);             // (as kmhg_query_run)
      check_query_args(L, k);
    }
    DeviceGuard g(idx->device);
    hipStream_t s = lib_stream();
    DBuf<uint8_t> d(L + 16, s);
    L = h2d_cstring(d.p, seq, L, s);
    uint64_t H = 0;
    *out = records_blocks(idx, d.p, capped(idx, query_call(L, k)).on_rc(rc != 0), min_len, max_gap,
                          min_hits, s, &H);
    if (n_blocks) *n_blocks = (*out)->B;
    if (n_rows) *n_rows = (int64_t)H;
  });
}

int kmhg_rows_blocks(const void* d_rows, int64_t n_rows, int64_t min_len, int64_t max_gap,
                     int64_t min_hits, void* stream, kmhg_blocks** out, int64_t* n_blocks) {
  return guarded([&] {
    check_blocks_args(min_len, max_gap, min_hits, out);
    if (n_rows < 0 || n_rows > INT32_MAX) fail(KMHG_EINVAL, "bad row count");
    if (n_rows && !d_rows) fail(KMHG_EINVAL, "null argument");
    *out = rows_blocks(static_cast<const int2*>(d_rows), n_rows, min_len, max_gap, min_hits,
                       (hipStream_t)stream);
    if (n_blocks) *n_blocks = (*out)->B;
  });
}

int kmhg_query_blocks(kmhg_query* q, int64_t min_len, int64_t max_gap, int64_t min_hits,
                      kmhg_blocks** out, int64_t* n_blocks) {
  return guarded([&] {
    if (!q) fail(KMHG_EINVAL, "null argument");
    check_blocks_args(min_len, max_gap, min_hits, out);
    if (q->n_runs >= 0) fail(KMHG_EINVAL, "the query holds runs (kmhg_query_runs_device)");
    if (q->H > INT32_MAX) fail(KMHG_EINVAL, "bad row count");
    gather_parts(q);                    // a multi-device query's rows, on its home device
    DeviceGuard g(q->device);
    *out = rows_blocks(q->rows.p, q->H, min_len, max_gap, min_hits, q->stream);
    if (n_blocks) *n_blocks = (*out)->B;
  });
}

int kmhg_blocks_device(kmhg_blocks* b, const int32_t** d_blocks, int64_t* n_blocks) {
  return guarded([&] {
    if (!b || !d_blocks) fail(KMHG_EINVAL, "null argument");
    *d_blocks = b->B ? b->blocks.p : nullptr;
    if (n_blocks) *n_blocks = b->B;
  });
}

int kmhg_blocks_copy_device(kmhg_blocks* b, void* d_dst, void* stream) {
  return guarded([&] {
    if (!b) fail(KMHG_EINVAL, "null argument");
    if (!b->B) return;
    if (!d_dst) fail(KMHG_EINVAL, "null output");
    DeviceGuard dg(b->device);
    HIPC(hipMemcpyAsync(d_dst, b->blocks.p, (size_t)b->B * 16, hipMemcpyDeviceToDevice,
                        (hipStream_t)stream));
  });
}

int kmhg_blocks_fill(kmhg_blocks* b, int32_t* blocks) {
  return guarded([&] {
    if (!b) fail(KMHG_EINVAL, "null argument");
    if (!b->B) return;
    if (!blocks) fail(KMHG_EINVAL, "null output");
    DeviceGuard dg(b->device);
    d2h_host(blocks, b->blocks.p, (size_t)b->B * 16, lib_stream());
  });
}

int kmhg_blocks_free(kmhg_blocks* b) {
  return guarded([&] {
    if (!b) return;
    std::unique_ptr<kmhg_blocks> own(b);
    if (!b->B) return;
    DeviceGuard dg(b->device);
    // the caller keeps the stream it made the blocks on alive until here (as for a query)
    HIPC(hipStreamSynchronize(b->stream));
  });
}

// -------------------------------------------------------------------------- seq.kmer.chains
namespace {

void check_chain_params(int64_t max_dist, int64_t max_drift, int64_t min_hits) {
  const ChainRefusal r = chain_check_params(max_dist, max_drift, min_hits);
  if (r.code != KMHG_OK) fail(r.code, r.text);
}

// The chains of n_blocks > 0 blocks on the current device (kmhg_chains.hip; include/kmhgpu.h has
// the definition), into g: keys / sort / prep / pred / link / jump / sum / count, then emit and
// member.  Scratch is O(B) on `s`.  Waits for `s` once where the number of chains sizes the result
// -- the input faults are answered there too: no pass leaves [0, B) whatever the blocks hold --
// and once more at the end: `s` is idle when it returns.
void chain_blocks(const int32_t* blocks, int64_t n_blocks, int64_t max_dist, int64_t max_drift,
                  int64_t min_hits, hipStream_t s, kmhg_chains* g) {
  const uint32_t B = (uint32_t)n_blocks;
  const uint32_t dist = chain_limit(max_dist), drift = chain_limit(max_drift);
  const uint32_t mh = chain_min_hits(min_hits);
  HIPC(hipGetDevice(&g->device));
  g->stream = s;
  ReleaseGroup rg(s);
  PinnedRec hrec = PinnedPool::get().take();
  GiveBack give_back{hrec, s};
  BuildMeta* hm = hrec.meta;            // n_small / n_large: the faults; n_pairs: chains
  const uint64_t nt = ((uint64_t)B + TILE - 1) / TILE;
  size_t tb = 0;
  HIPC(chains_sort_temp_bytes(B, &tb));
  DBuf<uint64_t> keys(2 * (size_t)B, s);            // {ei << 32 | b}: as made, sorted
  DBuf<uint8_t> temp(std::max<size_t>(tb, 16), s);
  DBuf<uint64_t> links(2 * (size_t)B, s);           // pred, child
  DBuf<uint32_t> win(2 * (size_t)B, s);             // {lo, hi} per block
  DBuf<int32_t> sej((size_t)B, s);                  // ej by sorted rank
  DBuf<int32_t> ends(2 * (size_t)B, s);             // {ei, ej} of the last block, per first block
  DBuf<uint32_t> nums(4 * (size_t)B, s);            // up; hits, count, cid (zeroed)
  DBuf<uint64_t> tiles(nt + scan_u64_scratch(nt), s);
  uint64_t *skey = keys.p + B, *pred = links.p, *child = links.p + B;
  uint32_t *up = nums.p, *hits = nums.p + B, *count = nums.p + 2 * (size_t)B,
           *cid = nums.p + 3 * (size_t)B;
  __atomic_store_n(&hm->n_small, 0u, __ATOMIC_RELEASE);
  __atomic_store_n(&hm->n_large, 0u, __ATOMIC_RELEASE);
  LAUNCH("k_chains_keys", s, launch_chains_keys(blocks, B, keys.p, &hm->n_small, &hm->n_large, s));
  hipError_t sort_err = hipSuccess;
  LAUNCH("k_chains_sort", s, sort_err = launch_chains_sort(keys.p, B, skey, temp.p, tb, s));
  HIPC(sort_err);
  LAUNCH("k_chains_prep", s, launch_chains_prep(blocks, B, skey, dist, sej.p, win.p, s));
  HIPC(hipMemsetAsync(child, 0xFF, (size_t)B * 8, s));
  HIPC(hipMemsetAsync(hits, 0, (size_t)B * 12, s));
  LAUNCH("k_chains_pred", s,
         launch_chains_pred(blocks, B, skey, sej.p, win.p, dist, drift, pred, child, s));
  LAUNCH("k_chains_link", s, launch_chains_link(B, pred, child, up, s));
  for (int r = chain_rounds(B); r > 0; --r) LAUNCH("k_chains_jump", s, launch_chains_jump(B, up, s));
  LAUNCH("k_chains_sum", s, launch_chains_sum(blocks, B, up, child, hits, count, ends.p, s));
  LAUNCH("k_chains_order", s, launch_chains_count(B, up, hits, mh, tiles.p, s));
  LAUNCH("k_scan_tiles_u64", s, launch_scan_u64(tiles.p, nt, &hm->n_pairs, tiles.p + nt, s));
  HIPC(hipStreamSynchronize(s));
  const ChainRefusal rf = chain_fault_refusal(
      (__atomic_load_n(&hm->n_small, __ATOMIC_ACQUIRE) ? CHAIN_UNSORTED : 0u) |
      (__atomic_load_n(&hm->n_large, __ATOMIC_ACQUIRE) ? CHAIN_BAD_BLOCK : 0u));
  if (rf.code != KMHG_OK) fail(rf.code, rf.text);
  const uint64_t C = __atomic_load_n(&hm->n_pairs, __ATOMIC_ACQUIRE);
  if (C > B) fail(KMHG_EDEVICE, "more chains than blocks");
  g->member.reset(B);
  if (C) {
    g->chains.reset(6 * (size_t)C);
    LAUNCH("k_chains_order", s,
           launch_chains_emit(blocks, B, up, hits, count, ends.p, mh, tiles.p, C, g->chains.p, cid,
                              s));
  }
  LAUNCH("k_chains_member", s, launch_chains_member(B, up, cid, g->member.p, s));
  HIPC(hipStreamSynchronize(s));
  g->C = (int64_t)C;
  g->B = (int64_t)B;
  rg.synced = true;
}

struct QueryFree {
  void operator()(kmhg_query* q) const {
    try { free_query(q); } catch (const Error&) {}
  }
};

// seq.kmer.chains of a query on the index's device: the blocks by the rows route (query_device,
// then rows_blocks) or the row-free one (records_blocks), at min_hits = 1, kept in the handle and
// chained.  *H <- the hit total.  No block gives an empty handle.
kmhg_chains* query_chains(kmhg_index* idx, const uint8_t* d_seq, const QueryCall& c, bool row_free,
                          int64_t min_len, int64_t max_gap, int64_t max_dist, int64_t max_drift,
                          int64_t min_hits, hipStream_t s, uint64_t* H) {
  auto g = std::make_unique<kmhg_chains>();
  std::unique_ptr<kmhg_blocks> b;
  if (row_free) {
    b.reset(records_blocks(idx, d_seq, c, min_len, max_gap, 1, s, H));
  } else {
    if (!idx->canonical && idx->is_part == c.part && idx->sources)
      fail(KMHG_EINVAL, "blocks need a position index");
    std::unique_ptr<kmhg_query, QueryFree> q(query_device(idx, d_seq, c, s));
    *H = (uint64_t)q->H;
    if (q->H > INT32_MAX) fail(KMHG_EINVAL, "bad row count");
    b.reset(rows_blocks(q->rows.p, q->H, min_len, max_gap, 1, s));
    q.reset();                          // (the rows' stream is idle: rows_blocks ended in a wait)
  }
  g->holds_blocks = true;
  if (!b->B) return g.release();
  g->blocks.swap_with(b->blocks);
  chain_blocks(g->blocks.p, b->B, max_dist, max_drift, min_hits, s, g.get());
  return g.release();
}

void check_chains_args(int64_t min_len, int64_t max_gap, int64_t max_dist, int64_t max_drift,
                       int64_t min_hits, kmhg_chains** out) {
  if (!out) fail(KMHG_EINVAL, "null argument");
  if (min_len < 1) fail(KMHG_EINVAL, "min_len must be a positive integer");
  if (max_gap < 0) fail(KMHG_EINVAL, "max_gap must not be negative");
  check_chain_params(max_dist, max_drift, min_hits);
}

}  // namespace

int kmhg_blocks_chains(const void* d_blocks, int64_t n_blocks, int64_t max_dist, int64_t max_drift,
                       int64_t min_hits, void* stream, kmhg_chains** out, int64_t* n_chains) {
  return guarded([&] {
    if (!out) fail(KMHG_EINVAL, "null argument");
    check_chain_params(max_dist, max_drift, min_hits);
    const ChainRefusal r = chain_check_count(n_blocks);
    if (r.code != KMHG_OK) fail(r.code, r.text);
    if (n_blocks && !d_blocks) fail(KMHG_EINVAL, "null argument");
    if (n_blocks && (reinterpret_cast<uintptr_t>(d_blocks) & 15))
      fail(KMHG_EINVAL, "blocks must be 16-byte aligned");
    auto g = std::make_unique<kmhg_chains>();
    if (n_blocks)                         // (none: no device call, an empty result is host-only)
      chain_blocks(static_cast<const int32_t*>(d_blocks), n_blocks, max_dist, max_drift, min_hits,
                   (hipStream_t)stream, g.get());
    *out = g.release();
    if (n_chains) *n_chains = (*out)->C;
  });
}

int kmhg_chains_run_device(kmhg_index* idx, const void* d_seq, size_t L, int k, int rc,
                           int row_free, int64_t min_len, int64_t max_gap, int64_t max_dist,
                           int64_t max_drift, int64_t min_hits, void* stream, kmhg_chains** out,
                           int64_t* n_chains, int64_t* n_blocks, int64_t* n_rows) {
  return guarded([&] {
    if (!idx || !d_seq) fail(KMHG_EINVAL, "null argument");
    check_chains_args(min_len, max_gap, max_dist, max_drift, min_hits, out);
    const QueryCall c = capped(idx, query_call(L, k)).on_rc(rc != 0);
    DeviceGuard g(idx->device);
    uint64_t H = 0;
    *out = query_chains(idx, static_cast<const uint8_t*>(d_seq), c, row_free != 0, min_len,
                        max_gap, max_dist, max_drift, min_hits, (hipStream_t)stream, &H);
    if (n_chains) *n_chains = (*out)->C;
    if (n_blocks) *n_blocks = (*out)->B;
    if (n_rows) *n_rows = (int64_t)H;
  });
}

int kmhg_chains_run(kmhg_index* idx, const char* seq, size_t L, int k, int rc, int row_free,
                    int64_t min_len, int64_t max_gap, int64_t max_dist, int64_t max_drift,
                    int64_t min_hits, kmhg_chains** out, int64_t* n_chains, int64_t* n_blocks,
                    int64_t* n_rows) {
  return guarded([&] {
    if (!idx || !seq) fail(KMHG_EINVAL, "null argument");
    check_chains_args(min_len, max_gap, max_dist, max_drift, min_hits, out);
    if (L < H2D_SCAN_MIN || k < 1 || k > 31 || L >= (size_t)INT32_MAX) {
      L = effective_len(seq, L);             // (as kmhg_query_run)
      check_query_args(L, k);
    }
    DeviceGuard g(idx->device);
    hipStream_t s = lib_stream();
    DBuf<uint8_t> d(L + 16, s);
    L = h2d_cstring(d.p, seq, L, s);
    uint64_t H = 0;
    *out = query_chains(idx, d.p, capped(idx, query_call(L, k)).on_rc(rc != 0), row_free != 0, min_len,
                        max_gap, max_dist, max_drift, min_hits, s, &H);
    if (n_chains) *n_chains = (*out)->C;
    if (n_blocks) *n_blocks = (*out)->B;
    if (n_rows) *n_rows = (int64_t)H;
  });
}

int kmhg_chains_device(kmhg_chains* c, const int32_t** d_chains, int64_t* n_chains,
                       const int32_t** d_member, const int32_t** d_blocks, int64_t* n_blocks) {
  return guarded([&] {
    if (!c || !d_chains) fail(KMHG_EINVAL, "null argument");
    *d_chains = c->C ? c->chains.p : nullptr;
    if (n_chains) *n_chains = c->C;
    if (d_member) *d_member = c->B ? c->member.p : nullptr;
    if (d_blocks) *d_blocks = c->B && c->holds_blocks ? c->blocks.p : nullptr;
    if (n_blocks) *n_blocks = c->B;
  });
}

int kmhg_chains_copy_device(kmhg_chains* c, void* d_chains, void* d_member, void* d_blocks,
                            void* stream) {
  return guarded([&] {
    if (!c) fail(KMHG_EINVAL, "null argument");
    if (d_blocks && !c->holds_blocks) fail(KMHG_EINVAL, "the handle holds no blocks");
    if (!c->B) return;
    if ((c->C && !d_chains) || !d_member) fail(KMHG_EINVAL, "null output");
    DeviceGuard dg(c->device);
    if (c->C)
      HIPC(hipMemcpyAsync(d_chains, c->chains.p, (size_t)c->C * 24, hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
    HIPC(hipMemcpyAsync(d_member, c->member.p, (size_t)c->B * 4, hipMemcpyDeviceToDevice,
                        (hipStream_t)stream));
    if (d_blocks)
      HIPC(hipMemcpyAsync(d_blocks, c->blocks.p, (size_t)c->B * 16, hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
  });
}

int kmhg_chains_fill(kmhg_chains* c, int32_t* chains) {
  return guarded([&] {
    if (!c) fail(KMHG_EINVAL, "null argument");
    if (!c->C) return;
    if (!chains) fail(KMHG_EINVAL, "null output");
    DeviceGuard dg(c->device);
    d2h_host(chains, c->chains.p, (size_t)c->C * 24, lib_stream());
  });
}

int kmhg_chains_member_fill(kmhg_chains* c, int32_t* member, int32_t* blocks) {
  return guarded([&] {
    if (!c) fail(KMHG_EINVAL, "null argument");
    if (blocks && !c->holds_blocks) fail(KMHG_EINVAL, "the handle holds no blocks");
    if (!c->B) return;
    if (!member) fail(KMHG_EINVAL, "null output");
    DeviceGuard dg(c->device);
    d2h_host(member, c->member.p, (size_t)c->B * 4, lib_stream());
    if (blocks) d2h_host(blocks, c->blocks.p, (size_t)c->B * 16, lib_stream());
  });
}

int kmhg_chains_free(kmhg_chains* c) {
  return guarded([&] {
    if (!c) return;
    std::unique_ptr<kmhg_chains> own(c);
    if (!c->B) return;
    DeviceGuard dg(c->device);
    // the caller keeps the stream it made the chains on alive until here (as for a query)
    HIPC(hipStreamSynchronize(c->stream));
  });
}

// -------------------------------------------------------------------------- seq.kmer.raster
namespace {

static RasterFrame checked_frame(const int64_t* frame) {
  const RasterFrame f = raster_frame(frame);
  const RasterRefusal r = raster_check_frame(f);
  if (r.code != KMHG_OK) fail(r.code, r.text);
  return f;
}

static size_t raster_cells(const RasterFrame& f) { return (size_t)(f.n_i * f.n_j); }

static void raster_rows(const int2* rows, int64_t n_rows, const RasterFrame& f, uint32_t* d_out,
                        hipStream_t s) {
  HIPC(hipMemsetAsync(d_out, 0, raster_cells(f) * 4, s));
  if (n_rows)
    LAUNCH("k_raster_rows", s, launch_raster_rows(rows, (uint64_t)n_rows, raster_dev(f), d_out, s));
  HIPC(hipGetLastError());
}

// The row-free route: query_device's checks and probe, then every hit added into its cell from
// the window records (k_raster_records) where query_device scans the tile totals into row
// offsets and writes the rows.  No row buffer, no exact-size re-emit and no 2^31 limit: the tile
// totals are summed only for the hit total, which is returned.  Synchronous.
static uint64_t raster_device(kmhg_index* idx, const uint8_t* d_seq, const QueryCall& c,
                              const RasterFrame& f, uint32_t* d_out, hipStream_t s) {
  ReleaseGroup rg(s);
  records_index(idx, c, s, nullptr);
  HIPC(hipMemsetAsync(d_out, 0, raster_cells(f) * 4, s));
  const int64_t Nw = c.w1 - c.w0;
  if (Nw <= 0) {
    HIPC(hipStreamSynchronize(s));
    return 0;
  }
  QueryRecords r;
  PinnedRec hrec = PinnedPool::get().take();
  GiveBack give_back{hrec, s};
  uint64_t* total = &hrec.meta->n_kmers;
  probe_records(idx, d_seq, c, total, s, r);
  if ((uint64_t)f.bin_i * (uint64_t)f.bin_j >= (1ull << 32)) {
    // only such a frame can overflow a cell: the total is read before any add
    HIPC(hipStreamSynchronize(s));
    if (raster_may_overflow(f, __atomic_load_n(total, __ATOMIC_ACQUIRE)))
      fail(KMHG_EOVERFLOW, "a raster cell could exceed 2^32-1 rows");
  }
  LAUNCH("k_raster_records", s,
         launch_raster_records(r.qrec.p, r.qmulti.p, Nw, c.w0, c.k, idx->positions.p, raster_dev(f),
                               d_out, s));
  HIPC(hipStreamSynchronize(s));
  rg.synced = true;
  return __atomic_load_n(total, __ATOMIC_ACQUIRE);
}

}  // namespace

int kmhg_rows_raster(const void* d_rows, int64_t n_rows, const int64_t frame[6], void* d_out,
                     void* stream) {
  return guarded([&] {
    if (!frame || !d_out) fail(KMHG_EINVAL, "null argument");
    const RasterFrame f = checked_frame(frame);
    if (n_rows < 0 || n_rows > INT32_MAX) fail(KMHG_EINVAL, "bad row count");
    if (n_rows && !d_rows) fail(KMHG_EINVAL, "null argument");
    raster_rows(static_cast<const int2*>(d_rows), n_rows, f, static_cast<uint32_t*>(d_out),
                (hipStream_t)stream);
  });
}

int kmhg_query_raster(kmhg_query* q, const int64_t frame[6], void* d_out, void* stream) {
  return guarded([&] {
    if (!q || !frame || !d_out) fail(KMHG_EINVAL, "null argument");
    const RasterFrame f = checked_frame(frame);
    if (q->n_runs >= 0) fail(KMHG_EINVAL, "the query holds runs (kmhg_query_runs_device)");
    if (q->H > INT32_MAX) fail(KMHG_EINVAL, "bad row count");
    gather_parts(q);                    // a multi-device query's rows, on its home device
    DeviceGuard g(q->device);
    hipStream_t s = (hipStream_t)stream;
    if (s != q->stream) {               // order after the emit kernel queued on q->stream
      hipEvent_t ev;
      HIPC(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      HIPC(hipEventRecord(ev, q->stream));
      HIPC(hipStreamWaitEvent(s, ev, 0));
      HIPC(hipEventDestroy(ev));
    }
    raster_rows(q->rows.p, q->H, f, static_cast<uint32_t*>(d_out), s);
  });
}

int kmhg_raster_run_device(kmhg_index* idx, const void* d_seq, size_t L, int k, int rc,
                           const int64_t frame[6], void* d_out, void* stream, int64_t* n_rows) {
  return guarded([&] {
    if (!idx || !d_seq || !frame || !d_out) fail(KMHG_EINVAL, "null argument");
    const RasterFrame f = checked_frame(frame);
    const QueryCall c = capped(idx, query_call(L, k)).on_rc(rc != 0);
    DeviceGuard g(idx->device);
    const uint64_t H = raster_device(idx, static_cast<const uint8_t*>(d_seq), c, f,
                                     static_cast<uint32_t*>(d_out), (hipStream_t)stream);
    if (n_rows) *n_rows = (int64_t)H;
  });
}

int kmhg_raster_run(kmhg_index* idx, const char* seq, size_t L, int k, int rc,
                    const int64_t frame[6], uint32_t* out, int64_t* n_rows) {
  return guarded([&] {
    if (!idx || !seq || !frame || !out) fail(KMHG_EINVAL, "null argument");
    const RasterFrame f = checked_frame(frame);
    if (L < H2D_SCAN_MIN || k < 1 || k > 31 || L >= (size_t)INT32_MAX) {
      L = effective_len(seq, L);             // (as kmhg_query_run)
      check_query_args(L, k);
    }
    DeviceGuard g(idx->device);
    hipStream_t s = lib_stream();
    DBuf<uint8_t> d(L + 16, s);
    DBuf<uint32_t> m(raster_cells(f), s);
    L = h2d_cstring(d.p, seq, L, s);
    const uint64_t H = raster_device(idx, d.p, capped(idx, query_call(L, k)).on_rc(rc != 0), f, m.p, s);
    d2h_host(out, m.p, raster_cells(f) * 4, s);
    if (n_rows) *n_rows = (int64_t)H;
  });
}

int kmhg_image_sizes_get(const kmhg_index* cidx, kmhg_image_sizes* sz, int64_t header[8]) {
  return guarded([&] {
    if (!cidx || !sz || !header) fail(KMHG_EINVAL, "null argument");
    kmhg_index* idx = const_cast<kmhg_index*>(cidx);   // completes a pending build
    if (idx->sources) fail(KMHG_EINVAL, "index images hold position indices only");
    if (idx->is_part) fail(KMHG_EINVAL, "a part index is exported with kmhg_part_export");
    DeviceGuard g(idx->device);
    finish_build(idx);
    sz->table_bytes = (int64_t)(idx->slots() * sizeof(Slot));
    sz->positions_bytes = (int64_t)(idx->N * 4);
    sz->codes_bytes = idx->dcodes.p ? (int64_t)(diag_block_words(idx->L - idx->k + 1) * 8) : 0;
    header[0] = idx->k; header[1] = idx->L;
    header[2] = ((int64_t)idx->geom.nb << 32) | idx->geom.capb;
    header[3] = (int64_t)idx->U; header[4] = (int64_t)idx->N; header[5] = (int64_t)idx->P;
    header[6] = idx->max_n; header[7] = 0x6B6D6867;   // 'kmhg'
  });
}

int kmhg_image_export(const kmhg_index* cidx, void* d_table, void* d_positions, void* d_codes,
                      void* stream) {
  return guarded([&] {
    if (!cidx) fail(KMHG_EINVAL, "null index");
    kmhg_index* idx = const_cast<kmhg_index*>(cidx);
    if (idx->sources) fail(KMHG_EINVAL, "index images hold position indices only");
    if (idx->sampling > 1) fail(KMHG_EINVAL, "index images do not carry a sampling");
    DeviceGuard g(idx->device);
    finish_build(idx);
    hipStream_t s = (hipStream_t)stream;   // caller stream; NULL = HIP null stream
    if (d_table) HIPC(hipMemcpyAsync(d_table, idx->table.p, idx->slots() * sizeof(Slot),
                                     hipMemcpyDeviceToDevice, s));
    if (d_positions && idx->N)
      HIPC(hipMemcpyAsync(d_positions, idx->positions.p, idx->N * 4, hipMemcpyDeviceToDevice, s));
    if (d_codes && idx->dcodes.p)
      HIPC(hipMemcpyAsync(d_codes, idx->dcodes.p, diag_block_words(idx->L - idx->k + 1) * 8,
                          hipMemcpyDeviceToDevice, s));
    HIPC(hipStreamSynchronize(s));
  });
}

int kmhg_image_import(const int64_t header[8], const void* d_table, const void* d_positions,
                      const void* d_codes, void* stream, kmhg_index** out) {
  return guarded([&] {
    if (!header || !out || header[7] != 0x6B6D6867) fail(KMHG_EINVAL, "bad index image header");
    auto idx = std::make_unique<kmhg_index>();
    HIPC(hipGetDevice(&idx->device));
    hipStream_t s = (hipStream_t)stream;
    idx->k = (int)header[0]; idx->L = header[1];
    idx->geom = Geom{(uint32_t)((uint64_t)header[2] >> 32), (uint32_t)(header[2] & 0xFFFFFFFF)};
    idx->U = (uint64_t)header[3]; idx->N = (uint64_t)header[4]; idx->P = (uint64_t)header[5];
    idx->max_n = (uint32_t)header[6];
    idx->table.reset(idx->slots());
    idx->positions.reset(idx->N);
    if (!d_table || (idx->N && !d_positions)) fail(KMHG_EINVAL, "null image buffer");
    HIPC(hipMemcpyAsync(idx->table.p, d_table, idx->slots() * sizeof(Slot),
                        hipMemcpyDeviceToDevice, s));
    if (idx->N)
      HIPC(hipMemcpyAsync(idx->positions.p, d_positions, idx->N * 4, hipMemcpyDeviceToDevice, s));
    if (d_codes) {   // the diagonal query path's code block (its uniq bits are derived on first use)
      const uint64_t w = diag_block_words(idx->L - idx->k + 1);
      idx->dcodes.reset(w);
      HIPC(hipMemcpyAsync(idx->dcodes.p, d_codes, w * 8, hipMemcpyDeviceToDevice, s));
    }
    HIPC(hipStreamSynchronize(s));
    *out = idx.release();
  });
}

int kmhg_check_lds_lane_order(uint64_t* out_of_order, uint64_t* checked) {
  return guarded([&] {
    if (!out_of_order || !checked) fail(KMHG_EINVAL, "null result pointer");
    DBuf<unsigned long long> res(2, nullptr);
    HIPC(hipMemsetAsync(res.p, 0, 2 * sizeof(unsigned long long), nullptr));
    launch_lane_order_check(res.p, nullptr);
    unsigned long long h[2] = {0, 0};
    HIPC(hipMemcpy(h, res.p, sizeof(h), hipMemcpyDeviceToHost));
    *out_of_order = h[0];
    *checked = h[1];
  });
}

int kmhg_timing_enable(int on) {
  Timing::get().on = on != 0;
  return KMHG_OK;
}

int kmhg_timing_select(const char* kernel) {
  return guarded([&] { Timing::get().only = kernel ? kernel : ""; });
}

int kmhg_timing_reset(void) {
  return guarded([&] {
    Timing::get().collect();
    Timing::get().acc.clear();
  });
}

int kmhg_timing_report(char* buf, size_t cap) {
  return guarded([&] {
    Timing& t = Timing::get();
    t.collect();
    std::string js = "{";
    bool first = true;
    for (auto& kv : t.acc) {
      char tmp[256];
      snprintf(tmp, sizeof tmp, "%s\"%s\": [%lld, %.6f]", first ? "" : ", ", kv.first.c_str(),
               (long long)kv.second.first, kv.second.second);
      js += tmp;
      first = false;
    }
    js += "}";
    if (!buf || cap < js.size() + 1) fail(KMHG_EINVAL, "timing report buffer too small");
    memcpy(buf, js.c_str(), js.size() + 1);
  });
}

int kmhg_bucket_place_counters(uint64_t out[3], int reset) {
  return guarded([&] {
    if (!out) fail(KMHG_EINVAL, "null result pointer");
    out[0] = out[1] = out[2] = 0;
#ifdef KMHG_TEST_BUILD
    std::lock_guard<std::mutex> lk(g_place_mu);
    if (!g_place_ctr) return;
    int dev = 0;
    HIPC(hipGetDevice(&dev));
    HIPC(hipSetDevice(g_place_dev));
    uint32_t h[3] = {0, 0, 0};
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h, g_place_ctr, sizeof(h), hipMemcpyDeviceToHost);
    if (e == hipSuccess && reset) e = hipMemset(g_place_ctr, 0, sizeof(h));
    (void)hipSetDevice(dev);
    hip_check(e, "bucket placement counters");
    for (int i = 0; i < 3; ++i) out[i] = h[i];
#else
    (void)reset;
#endif
  });
}

int kmhg_bid_pack_counters(uint64_t out[2], int reset) {
  return guarded([&] {
    if (!out) fail(KMHG_EINVAL, "null result pointer");
    out[0] = out[1] = 0;
#ifdef KMHG_TEST_BUILD
    for (int i = 0; i < 2; ++i)
      out[i] = reset ? g_bid_pack_ctr[i].exchange(0, std::memory_order_relaxed)
                     : g_bid_pack_ctr[i].load(std::memory_order_relaxed);
#else
    (void)reset;
#endif
  });
}

int kmhg_pool_trim(void) {
  return guarded([&] { DevicePool::get().trim(); });
}

int64_t kmhg_pool_cached_bytes(void) { return DevicePool::get().cached(); }

}  // extern "C"
