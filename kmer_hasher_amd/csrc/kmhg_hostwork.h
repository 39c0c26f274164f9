// kmhg_hostwork.h -- the readout's host-side work (host only: no HIP, any C++17 compiler).
//
// What the engine's host-pointer entry points do on CPU threads once the bytes have left the
// device: the worker pool, the striping of a range over it, the expansion of diagonal runs and of
// pair lists into rows, and the small pure helpers around them (huge-page spans, table capacity, a
// C string's length).  Nothing here reads the environment: the
// engine passes every choice in.  tools/asan/host_check runs all of it under ASan + UBSan and
// under ThreadSanitizer at shapes of a few rows (tests/test_host_work.py).
#pragma once
#include <sched.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace kmhg {

// Host worker pool for the host-side copies: HOST_WORKERS threads made on first use and kept,
// so a call that splits a few MB over threads does not pay their creation and join (8 threads:
// ~0.1-0.35 ms a round -- per 16-MB chunk of a staged copy before).  run(n, fn) runs fn(0) ..
// fn(n - 1), the calling thread taking tasks too, and returns when all are done; calls from
// several threads at once (a multi-device query's parts) share the workers.  No task may call
// run() itself.  fresh = true (GB-scale writes: the expansions) starts fresh threads instead: the
// kernel spreads new threads over the machine's memory controllers, while woken pool workers
// crowd near their waker (A/B in one run, profiles/r6al_pool_ab/: config 5's run expansion
// 18-21 ms fresh, 30-54 pooled; config 4's pair rows 108-112 fresh, 99-164 pooled).
constexpr uint64_t HOST_BIG_BYTES = 512u << 20;   // (config 2's 80 MB of rows: pooled 0.84-0.91
                                                  // ms, fresh 1.19-1.41; profiles/r6ak*, r6al*)
class HostPool {
 public:
  static constexpr int HOST_WORKERS = 15;        // + the calling thread = 16
  static HostPool& get() {
    static HostPool p;
    return p;
  }
  void run(int n, const std::function<void(int)>& fn, bool fresh = false) {
    if (n <= 1) {
      if (n == 1) fn(0);
      return;
    }
    if (fresh) {
      std::vector<std::thread> th;
      for (int i = 1; i < n; ++i) th.emplace_back(fn, i);
      fn(0);
      for (auto& t : th) t.join();
      return;
    }
    Job job{&fn, n};
    {
      std::lock_guard<std::mutex> g(mu_);
      if (workers_.empty()) start();
      jobs_.push_back(&job);
    }
    cv_.notify_all();
    work_on(job, false);                         // until every task is handed out
    {
      std::lock_guard<std::mutex> g(mu_);        // no worker takes the job from here on
      for (auto it = jobs_.begin(); it != jobs_.end(); ++it)
        if (*it == &job) {
          jobs_.erase(it);
          break;
        }
    }
    std::unique_lock<std::mutex> g(job.m);       // the job lives until its last worker is out
    job.cv.wait(g, [&] { return job.done == job.n && job.refs == 0; });
  }
  ~HostPool() {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : workers_) t.join();
  }

 private:
  struct Job {
    const std::function<void(int)>* fn;
    int n;
    std::atomic<int> next{0};
    int done = 0, refs = 0;                      // guarded by m (refs: workers inside)
    std::mutex m;
    std::condition_variable cv;
    Job(const std::function<void(int)>* f, int count) : fn(f), n(count) {}
  };
  void work_on(Job& job, bool worker) {
    int ran = 0;
    for (int i; (i = job.next.fetch_add(1)) < job.n; ++ran) (*job.fn)(i);
    std::lock_guard<std::mutex> g(job.m);
    job.done += ran;
    if (worker) --job.refs;
    if (job.done == job.n && job.refs == 0) job.cv.notify_all();
  }
  void start() {
    for (int w = 0; w < HOST_WORKERS; ++w)
      workers_.emplace_back([this] {
        for (;;) {
          Job* job = nullptr;
          {
            std::unique_lock<std::mutex> g(mu_);
            cv_.wait(g, [&] {
              while (!jobs_.empty() && jobs_.front()->next.load() >= jobs_.front()->n)
                jobs_.pop_front();                 // handed out completely
              return stop_ || !jobs_.empty();
            });
            if (stop_) return;
            job = jobs_.front();
            std::lock_guard<std::mutex> gj(job->m);
            ++job->refs;                           // (the caller waits for it)
          }
          work_on(*job, true);
        }
      });
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<Job*> jobs_;
  std::vector<std::thread> workers_;
  bool stop_ = false;
};

// [0, total) in T stripes of ceil(total / T) rounded up to `align` (a power of two), stripe t on
// task t of the pool: fn(a, b) for every stripe that is not empty.
template <class F>
void for_stripes(uint64_t total, int T, uint64_t align, bool fresh, F&& fn) {
  const uint64_t stripe = ((total + T - 1) / T + align - 1) & ~(align - 1);
  HostPool::get().run(T, [&](int t) {
    const uint64_t a = std::min(total, t * stripe), b = std::min(total, a + stripe);
    if (a < b) fn(a, b);
  }, fresh);
}

// Host threads for the expansion: it is bound by the host's write bandwidth, which more threads
// reach (box, 16 CPUs, config 5's 376 M rows: 4 threads 51 ms, 8 30 ms, 16 16.5 ms;
// profiles/r6y_runs_probe*.json): every CPU this process may run on, at most 16.
// (The host's later unmapping of the matrix grows with the threads that wrote it -- 80 MB: 2.5
// ms written by one thread, 5.2 by 16, profiles/r6af_release_probe.json -- but giving each thread
// 16 MB instead (5 threads at 80 MB) traded 0.85 ms of fill for 0.9 of release,
// profiles/r6ag_release.json: every thread is used from 1 MB of output per thread on.)
constexpr uint64_t EXPAND_MIN_BYTES = 1u << 20;
inline int expand_threads(uint64_t out_bytes) {
  static const int n = [] {
    cpu_set_t cs;
    CPU_ZERO(&cs);
    const int c = sched_getaffinity(0, sizeof(cs), &cs) == 0 ? CPU_COUNT(&cs) : 8;
    return std::max(1, std::min(16, c));
  }();
  return (int)std::max<uint64_t>(1, std::min<uint64_t>(n, out_bytes / EXPAND_MIN_BYTES));
}

// Query rows into a host matrix (kmhg_query_fill, the R matrix of seq.kmer.pos).  A dot plot's
// rows are diagonal runs -- (i, j), (i + 1, j + 1), ... (config 5: 133 rows per run) -- so from
// RUNS_HOST_MIN rows on, the device writes the runs (R_count, scan, R_emit: the sharded
// query's gather format), 12 B per run cross PCIe into a pinned buffer, and host threads
// expand them into dst: the link carries ~1/90 of the bytes and the host's memory bandwidth
// writes the rows.  Rows that do not shrink RUNS_HOST_GAIN-fold (multi-hit windows) are copied
// as they are.
constexpr uint64_t RUNS_HOST_MIN = 1u << 19;           // rows (4 MB)
constexpr uint64_t RUNS_HOST_GAIN = 4;

// rows [r0, r1) of the H rows that the n runs {first row, i0, j0} stand for, into dst (2 x int32
// per row, indexed by row)
inline void expand_runs_range(const int32_t* runs, uint64_t n, uint64_t H, uint64_t r0,
                              uint64_t r1, int32_t* dst) {
  uint64_t lo = 0, hi = n;                            // the run covering r0
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if ((uint64_t)(uint32_t)runs[3 * mid] <= r0) lo = mid; else hi = mid;
  }
  uint64_t r = r0;
  for (uint64_t q = lo; r < r1; ++q) {
    const uint64_t st = (uint32_t)runs[3 * q];
    const uint32_t i0 = (uint32_t)runs[3 * q + 1], j0 = (uint32_t)runs[3 * q + 2];
    const uint64_t e = std::min(r1, q + 1 < n ? (uint64_t)(uint32_t)runs[3 * q + 3] : H);
    uint32_t* o = reinterpret_cast<uint32_t*>(dst) + 2 * r;
    for (uint32_t d = (uint32_t)(r - st); r < e; ++r, ++d, o += 2) {
      o[0] = i0 + d;
      o[1] = j0 + d;
    }
  }
}
// all H rows on T threads (fresh ones from HOST_BIG_BYTES of rows on, or when `fresh` asks)
inline void expand_runs_host(const int32_t* runs, uint64_t n, uint64_t H, int32_t* dst, int T,
                             bool fresh = false) {
  for_stripes(H, T, 512, fresh || H * 8 >= HOST_BIG_BYTES,
              [=](uint64_t a, uint64_t b) { expand_runs_range(runs, n, H, a, b, dst); });
}

// kmer.pos's pair rows into a host matrix (the R API's readout).  A pair row is {key label,
// position j, position q} for every j < q of a repeated key's list -- P rows from the lists'
// ~N positions (config 4: 686 M rows, 8.2 GB, from 40 M positions) -- so from HOST_PAIRS_MIN
// rows on, the lists and their keys' offsets cross PCIe (pkeys, pair_off, rinfo, positions:
// ~0.4 GB at config 4) and host threads write the rows, each from its stripe's first pair on.
constexpr uint64_t HOST_PAIRS_MIN = 1u << 22;           // rows (48 MB)
struct RowInfo { uint32_t x, y; };   // {count, aux} of a row's slot: the device's uint2

// pairs of a key with n positions that start before list entry j
inline uint64_t pairs_before(uint64_t n, uint64_t j) { return j * (2 * n - j - 1) / 2; }
// the first entry of pair t of a key with n >= 2 positions, t < n (n - 1) / 2: the largest
// j <= n - 2 with pairs_before(n, j) <= t, as V_read_pairs
inline uint64_t pair_start(uint64_t n, uint64_t t) {
  if (!t) return 0;
  const double dn = 2.0 * (double)n - 1.0, disc = dn * dn - 8.0 * (double)t;
  uint64_t j = (uint64_t)std::max(0.0, (dn - std::sqrt(std::max(disc, 0.0))) * 0.5);
  j = std::min<uint64_t>(j, n - 2);
  while (j > 0 && pairs_before(n, j) > t) --j;
  while (j + 1 <= n - 2 && pairs_before(n, j + 1) <= t) ++j;
  return j;
}
// pair rows [r0, r1) of the P rows into out (3 x int32 per row, indexed by row): repeated key m
// of M is row pk[m] of the readout order, its pairs start at row po[m], its list is the ri[].x
// entries of ps that end at ri[].y
inline void expand_pairs_range(const uint32_t* pk, const uint64_t* po, uint64_t M,
                               const RowInfo* ri, const int32_t* ps, uint64_t r0, uint64_t r1,
                               int32_t* out) {
  uint64_t m = (uint64_t)(std::upper_bound(po, po + M, r0) - po) - 1;
  uint64_t t = r0 - po[m], r = r0;
  while (r < r1) {
    const uint32_t c = pk[m];
    const uint64_t n = ri[c].x;
    const int32_t* lst = ps + (ri[c].y - n);
    uint64_t j = pair_start(n, t);
    uint64_t q = j + 1 + (t - pairs_before(n, j));
    const int32_t lab = (int32_t)(c + 1);
    for (; j + 1 < n && r < r1; ++j, q = j + 1) {
      const int32_t pj = lst[j];
      const uint64_t qe = std::min<uint64_t>(n, q + (r1 - r));
      int32_t* o = out + 3 * r;
      for (uint64_t x = q; x < qe; ++x, o += 3) {
        o[0] = lab;
        o[1] = pj;
        o[2] = lst[x];
      }
      r += qe - q;
    }
    ++m;
    t = 0;
  }
}
// all P rows on T threads (fresh ones from HOST_BIG_BYTES of rows on, or when `fresh` asks)
inline void expand_pairs_host(const uint32_t* pk, const uint64_t* po, uint64_t M,
                              const RowInfo* ri, const int32_t* ps, uint64_t P, int32_t* out,
                              int T, bool fresh = false) {
  for_stripes(P, T, 1, fresh || P * 12 >= HOST_BIG_BYTES, [=](uint64_t a, uint64_t b) {
    expand_pairs_range(pk, po, M, ri, ps, a, b, out);
  });
}

// The whole 2-MB spans inside [dst, dst + bytes), the ones a huge-page hint can cover; nothing
// (len 0) below two spans of bytes.
constexpr size_t HUGE_SPAN = 2u << 20;
struct Span { uintptr_t begin; size_t len; };
inline Span huge_span(const void* dst, size_t bytes) {
  if (bytes < 2 * HUGE_SPAN) return {0, 0};
  const uintptr_t m = ~(uintptr_t)(HUGE_SPAN - 1), d = reinterpret_cast<uintptr_t>(dst);
  const uintptr_t a = (d + HUGE_SPAN - 1) & m, b = (d + bytes) & m;
  return b > a ? Span{a, (size_t)(b - a)} : Span{0, 0};
}

// The hash table is sized from the number of windows (an upper bound on distinct k-mers) for a
// load factor <= 0.7; capacity is not a power of two (slot = mulhi(hash, cap)).
inline uint64_t table_capacity(int64_t Nw) {
  uint64_t cap = (uint64_t)((double)Nw / 0.7) + 16;
  return (cap + 7) & ~7ull;
}

inline size_t effective_len(const char* seq, size_t L) {   // a C string ends at its first NUL
  const void* z = memchr(seq, 0, L);
  return z ? (size_t)((const char*)z - seq) : L;
}

}  // namespace kmhg
