// tools/asan/host_check.cpp -- the host-side C/C++ of the engine and of the oracle under
// AddressSanitizer + UndefinedBehaviorSanitizer (the reference itself was built
// with fortify / stack protection, src/debug.sh:17-23).  Built by tools/asan/Makefile, driven by
// tests/test_asan_host.py (CPU only).  What runs here is exactly the source the product and the
// checker compile: kmhg_fastx.h (the FASTA/FASTQ reader that parses untrusted input),
// kmhg_khash.h (the khash row-order replay), kmhg_plan.h (the partitioned build's plan),
// kmhg_hostwork.h (the readout's worker pool, stripes and row expansions), kmhg_reads.h (the host
// side of read counting), kmhg_pool.h (the device block pool, over a fake device),
// kmhg_querycall.h (the query entries' calls, rules and multi-device split),
// oracle/kmer_oracle.c and oracle/sh_oracle.c.  host_check_tsan is this file under
// ThreadSanitizer (tests/test_host_work.py, tests/test_pool_host.py).
//
//   host_check fastx <path> <max_records>   one line per record: R <len> <has_qual> <fnv seq>
//                                           <fnv qual>, then E <last return code>
//   host_check khash <n> <seed>             replay n random distinct keys with kmhg_khash.h and
//                                           the oracle's orc_khash_order; "ok <fnv>" if equal
//   host_check index <path> <k>             orc_index_build + orc_query (self) of the file's
//                                           bytes: U N P maxn H <wsum rows>
//   host_check reads <path> <k> <min_q>     orc_read_kmers of every record: n <wsum keys>
//   host_check plan <request> [round=<device round>] [KMHG_<knob>=<value> ...]
//                                           plan_build's plan, one line of field=value.  Request:
//                                           seq L=<chars> k=<k> [codes=0|1] [part=<p> n_parts=<n>]
//                                           | keys n=<keys> k=<k> | count n=<keys> k=<k> spread=<s>
//   host_check plan @<file>                 one plan per line of the file (the same arguments)
// kmhg_hostwork.h; the .bin files are raw little-endian arrays, outputs are the rows:
//   host_check stripes <total> <T> <align>  for_stripes' bounds, one "a b" line per stripe
//   host_check runs <runs.bin> <H> <T> <out.bin>           expand_runs_host on T threads
//   host_check runs-split <runs.bin> <H> <out.bin>         expand_runs_range over [0, c) and
//                                           [c, H) for every cut c; fails on the first output
//                                           that differs from the first cut's
//   host_check pairs <pk.bin> <po.bin> <ri.bin> <ps.bin> <T> <out.bin>     expand_pairs_host
//   host_check pairs-split <pk.bin> <po.bin> <ri.bin> <ps.bin> <out.bin>   as runs-split
//   host_check pair-start <file of "n t" lines>            pair_start's j, one per line
//   host_check pool <callers> <jobs> <max_tasks> <fresh 0|1>   caller threads submit jobs of
//                                           0 .. max_tasks tasks to HostPool at once; each task
//                                           adds its index to its job's sum; "ok" if all are right
//   host_check misc span=<address>,<bytes> | class=<bytes> | cap=<windows> | len=<hex bytes> ...
//                                           huge_span, pool_size_class (kmhg_pool.h),
//                                           table_capacity, effective_len: one line per argument
// kmhg_reads.h (tests/test_reads_host.py):
//   host_check read-call rp|sh1 <ints...>   read_call_rp / read_call_sh1 of the 8 / 6 parameters:
//                                           "err=<code> msg=<text>" or the decoded fields
//   host_check read-batches <span_max> <file of read lengths>   read_batches: "err=.. msg=.." or
//                                           one "i0 i1" line per range
//   host_check reads-longer <k> <fastx>     read_fastx at k = 0, then reads_longer_than(k): same
//                                           (1: the object itself came back), n, off, hasq and FNV
//                                           sums of seq and qual
//   host_check read-fastx <fastx> <k> <max_reads> <batch>   read_fastx flushing from <batch>
//                                           bases on: "B <reads> <bases>" per flush, then "T" with
//                                           the return value, the records, and every kept read's
//                                           length and has_qual with FNV sums over all batches
//   host_check spectrum-status <S> <comb,...> <comb_inner,...>   spectrum_status
// kmhg_querycall.h (tests/test_query_host.py), one field=value line per call:
//   host_check query call <L> <k> [<w_begin> <w_end>]   query_call / query_call_range: "err=<code>
//                                           msg=<text>" or the call's fields
//   host_check query rules guess=<Nw> | runs_pay=<H>,<NR> | redo=<H>,<cap> |
//                          diag=<kq>,<index k>,<sources>,<index windows>,<U>,<codes 0|1>,<knob 0|1> ...
//                                           query_rows_guess, runs_pay, needs_exact_redo,
//                                           diag_eligible: one line per argument
//   host_check query devices <text> <n>     parse_device_list: "err=.. msg=.." or devices=<d,...>
//   host_check query shards <L> <k> <G>     shard_windows and shard_chars of every part: w0 w1 c0 c1
//   host_check query offsets <H,...>        part_offsets: total and off
// kmhg_pool.h (tests/test_pool_host.py): BlockPool over FakeDev, whose blocks are malloc'ed bytes
// and whose events are the integers 1, 2, ... in the order they were made
//   host_check pool <script>                one operation per line of the file, one line of state
//                                           after each (pool_line below).  Operations:
//                                             knobs <depth> <best_fit 0|1>   (first line only)
//                                             dev <d>                 the thread's current device
//                                             alloc <name> <bytes>    the block is called <name>
//                                             release <name>|null|unknown [<stream>]   with a
//                                                                     stream: stream-ordered
//                                             group_begin <stream> | synced | group_end
//                                             own_event <stream>      an event of the caller's,
//                                                                     made and recorded (counted)
//                                             adopt <event>           the open group adopts it
//                                             complete <event>        the event has completed
//                                             fail alloc-oom|alloc-error|event|record <n>   the
//                                                                     next n such calls fail
//                                             trim | cached
//                                           and, for same-stream reuse and the run-ahead bound
//                                           (tests/test_pool_stream_reuse.py):
//                                             alloc_on <name> <bytes> <stream>   first used on
//                                                                     <stream> (alloc(bytes, stream))
//                                             dones                   ret = the backend's event
//                                                                     queries so far
//                                             ahead <n>               RecordPool's bound (before
//                                                                     the first rec_take; default 2)
//                                             rec_take <name>         ret = <event>:<free>:<pending>
//                                                                     of the record pool after it
//                                             rec_give <name> [<stream>]   with a stream: its event
//                                                                     recorded there, in flight
//   host_check pool threads <T> <ops>       T threads of <ops> mixed alloc / release / group
//                                           operations over three classes while another thread
//                                           completes the events; "ok" if every block is
//                                           accounted for at the end
//   host_check pool stream-threads <T> <ops>   the same, each thread asking for its blocks on its
//                                           own stream (same-stream reuse) and taking records
//                                           from one RecordPool
#include <cinttypes>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <type_traits>
#include <vector>

#include "../../kmer_hasher_amd/csrc/kmhg_fastx.h"
#include "../../kmer_hasher_amd/csrc/kmhg_khash.h"
#include "../../kmer_hasher_amd/csrc/kmhg_plan.h"
#include "../../kmer_hasher_amd/csrc/kmhg_hostwork.h"
#include "../../kmer_hasher_amd/csrc/kmhg_pool.h"
#include "../../kmer_hasher_amd/csrc/kmhg_reads.h"
#include "../../kmer_hasher_amd/csrc/kmhg_querycall.h"

extern "C" {
long orc_windows(const char* seq, long L, int k, uint64_t* keys, int32_t* s, int32_t* e);
long orc_index_build(const char* seq, long L, int k, uint64_t* ukeys, int32_t* counts,
                     int64_t* offsets, int32_t* positions, long* n_out, int64_t* pairs_out,
                     int32_t* maxn);
int64_t orc_query(const uint64_t* ukeys, const int32_t* counts, const int64_t* offsets,
                  const int32_t* positions, long U, const char* seq, long L, int kq,
                  int32_t* rows);
long orc_khash_order(const uint64_t* keys, long U, int64_t* order_out);
long orc_read_kmers(const unsigned char* seq, const unsigned char* qual, long len, int k,
                    int min_q, uint64_t* out);
}

static uint64_t fnv(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

// order-sensitive digest of an int array, vectorizable on the Python side:
// sum_i x_i * (i * 0x9E3779B97F4A7C15 + 1) mod 2^64 (x_i as unsigned 64-bit)
template <class T>
static uint64_t wsum(const T* x, size_t n) {
  uint64_t h = 0;
  for (size_t i = 0; i < n; ++i)
    h += (uint64_t)(std::make_unsigned_t<T>)x[i] * ((uint64_t)i * 0x9E3779B97F4A7C15ull + 1);
  return h;
}

static std::string slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  std::string s;
  char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
  fclose(f);
  return s;
}

static int cmd_fastx(const char* path, long max_records) {
  kmhg::FastxReader rd(path);
  if (!rd.ok()) { printf("E open\n"); return 0; }
  std::string sq, ql;
  bool hq = false;
  int rc = 0;
  for (long i = 0; i < max_records; ++i) {
    rc = rd.read(sq, ql, hq);
    if (rc < 0) break;
    printf("R %zu %d %016" PRIx64 " %016" PRIx64 "\n", sq.size(), hq ? 1 : 0,
           fnv(sq.data(), sq.size()), fnv(ql.data(), ql.size()));
  }
  printf("E %d\n", rc);
  return 0;
}

static uint64_t splitmix(uint64_t& x) {
  uint64_t z = (x += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static int cmd_khash(long n, uint64_t seed) {
  std::vector<uint64_t> keys;
  std::set<uint64_t> seen;
  uint64_t x = seed;
  while ((long)keys.size() < n) {
    // structured keys (2-bit DNA codes of k <= 31 plus a few near-duplicates) and random ones
    uint64_t v = splitmix(x);
    if (keys.size() % 3 == 0) v &= (1ull << 42) - 1;
    if (keys.size() % 7 == 1 && !keys.empty()) v = keys.back() ^ 1;
    if (seen.insert(v).second) keys.push_back(v);
  }
  const std::vector<uint32_t> a = kmhg::khash_bucket_order(keys);
  std::vector<int64_t> b((size_t)n + 1);
  const long m = orc_khash_order(keys.data(), n, b.data());
  if (m != (long)a.size()) { printf("size %ld %zu\n", m, a.size()); return 1; }
  for (long i = 0; i < m; ++i)
    if ((int64_t)a[(size_t)i] != b[(size_t)i]) { printf("diff at %ld\n", i); return 1; }
  printf("ok %016" PRIx64 "\n", fnv(a.data(), a.size() * 4));
  return 0;
}

static int cmd_index(const char* path, int k) {
  const std::string s = slurp(path);
  const long L = (long)s.size();
  std::vector<uint64_t> keys((size_t)L + 1);
  std::vector<int32_t> counts((size_t)L + 1), pos((size_t)L + 1);
  std::vector<int64_t> offs((size_t)L + 2);
  long N = 0;
  int64_t P = 0;
  int32_t mx = 0;
  const long U = orc_index_build(s.data(), L, k, keys.data(), counts.data(), offs.data(),
                                 pos.data(), &N, &P, &mx);
  if (U < 0) return 1;
  const int kq = k > 31 ? 31 : k;
  int64_t H = 0;
  uint64_t h = 0;
  if (L > kq) {
    H = orc_query(keys.data(), counts.data(), offs.data(), pos.data(), U, s.data(), L, kq,
                  nullptr);
    std::vector<int32_t> rows((size_t)(2 * H + 1));
    orc_query(keys.data(), counts.data(), offs.data(), pos.data(), U, s.data(), L, kq,
              rows.data());
    h = wsum(rows.data(), (size_t)(2 * H));
  }
  printf("%ld %ld %" PRId64 " %d %" PRId64 " %016" PRIx64 "\n", U, N, P, mx, H, h);
  return 0;
}

static int cmd_reads(const char* path, int k, int min_q) {
  kmhg::FastxReader rd(path);
  if (!rd.ok()) return 1;
  std::string sq, ql;
  bool hq = false;
  uint64_t h = 0;
  long n = 0;
  std::vector<uint64_t> all;
  while (rd.read(sq, ql, hq) >= 0) {
    if ((long)sq.size() <= k) continue;
    std::vector<uint64_t> out(sq.size() - k + 1);
    const long m = orc_read_kmers((const unsigned char*)sq.data(),
                                  hq ? (const unsigned char*)ql.data() : nullptr,
                                  (long)sq.size(), k, min_q, out.data());
    all.insert(all.end(), out.begin(), out.begin() + m);
    n += m;
  }
  h = wsum(all.data(), all.size());
  printf("%ld %016" PRIx64 "\n", n, h);
  return 0;
}

// one request line -> one line with the plan's fields; false: bad arguments
static bool plan_line(const std::vector<std::string>& a) {
  using namespace kmhg;
  if (a.empty()) return false;
  long long L = 0, n = 0, k = 0, codes = 1, part = 0, n_parts = 0, spread = 1, round = 0;
  BuildKnobs kn;
  for (size_t i = 1; i < a.size(); ++i) {
    const size_t eq = a[i].find('=');
    if (eq == std::string::npos) return false;
    const std::string name = a[i].substr(0, eq), v = a[i].substr(eq + 1);
    long long* dst = name == "L" ? &L : name == "n" ? &n : name == "k" ? &k
                     : name == "codes" ? &codes : name == "part" ? &part
                     : name == "n_parts" ? &n_parts : name == "spread" ? &spread
                     : name == "round" ? &round : nullptr;
    if (dst) *dst = atoll(v.c_str());
    else if (!set_build_knob(kn, name.c_str(), v.c_str())) return false;
  }
  BuildRequest rq;
  if (a[0] == "seq")
    rq = n_parts ? BuildRequest::sequence_part(L, (int)k, (uint32_t)part, (uint32_t)n_parts)
                 : BuildRequest::sequence(L, (int)k, codes != 0);
  else if (a[0] == "keys") rq = BuildRequest::key_stream((int)k, n);
  else if (a[0] == "count") rq = BuildRequest::count_keys((int)k, n, (int)spread);
  else return false;
  const BuildPlan P = plan_build(rq, kn, (uint32_t)round);
  if (P.err) { printf("err=%d msg=%s\n", P.err, P.msg); return true; }
  printf("err=0 empty=%d Nw=%lld ntiles=%u nb=%u b0=%u nbh=%u", P.empty_part ? 1 : 0,
         (long long)P.Nw, P.ntiles, P.geom.nb, P.geom.b0, P.geom.nbh);
  if (P.empty_part) { printf("\n"); return true; }
  printf(" R=%u passes=%u first=%u bid=%d bid_pack=%d aos=%d pack8=%d sh8=%d nseg8=%u ds=%d ds8=%d"
         " partc=%d co_auto=%d tags=%d nhist=%llu scan_tiles=%u key_bytes=%u,%u pos_array=%d,%d",
         P.R, P.passes, P.first_pass, P.bid, P.bid_pack, P.aos, P.pack8, P.sh8, P.nseg8, P.ds_on,
         P.ds8, P.partc, P.co_auto, P.want_tags, (unsigned long long)P.nhist, P.scan_tiles,
         P.key_bytes[0], P.key_bytes[1], P.pos_array[0], P.pos_array[1]);
  const int passes = (int)P.passes;
  printf(" fmt=");
  for (int p = -1; p < passes; ++p) printf("%s%s", p < 0 ? "" : ",", fmt_name(P.F(p)));
  printf(" side=");
  for (int p = -1; p < passes; ++p) printf("%s%d", p < 0 ? "" : ",", P.side(p));
  printf(" ds_out=");
  for (int p = -1; p < passes; ++p) printf("%s%d", p < 0 ? "" : ",", P.ds_out(p) ? 1 : 0);
  printf(" fused=");
  for (int p = 0; p < passes; ++p) printf("%s%d", p ? "," : "", P.fused((uint32_t)p) ? 1 : 0);
  printf("\n");
  return true;
}

static int cmd_plan(int argc, char** argv) {
  if (argc == 3 && argv[2][0] == '@') {
    std::ifstream f(argv[2] + 1);
    if (!f) { perror(argv[2] + 1); return 2; }
    std::string line;
    while (std::getline(f, line)) {
      std::istringstream is(line);
      std::vector<std::string> a;
      for (std::string w; is >> w;) a.push_back(w);
      if (!plan_line(a)) { fprintf(stderr, "bad plan arguments: %s\n", line.c_str()); return 2; }
    }
    return 0;
  }
  if (plan_line(std::vector<std::string>(argv + 2, argv + argc))) return 0;
  fprintf(stderr, "bad plan arguments\n");
  return 2;
}

// a raw file as an array of T, heap-allocated at its exact size (so ASan sees any overrun)
template <class T>
static std::vector<T> load(const char* path) {
  const std::string s = slurp(path);
  std::vector<T> v(s.size() / sizeof(T));
  memcpy(v.data(), s.data(), v.size() * sizeof(T));
  return v;
}

static int store(const char* path, const std::vector<int32_t>& v) {
  FILE* f = fopen(path, "wb");
  if (!f) { perror(path); return 2; }
  const size_t n = fwrite(v.data(), 4, v.size(), f);
  return (fclose(f) == 0 && n == v.size()) ? 0 : 2;
}

static int cmd_stripes(uint64_t total, int T, uint64_t align) {
  std::mutex mu;
  std::vector<std::pair<uint64_t, uint64_t>> got;
  kmhg::for_stripes(total, T, align, false, [&](uint64_t a, uint64_t b) {
    std::lock_guard<std::mutex> g(mu);
    got.push_back({a, b});
  });
  std::sort(got.begin(), got.end());
  for (auto& s : got) printf("%" PRIu64 " %" PRIu64 "\n", s.first, s.second);
  return 0;
}

// range(r0, r1, out) over [0, c) and [c, total) for every cut c: every output must equal the first
template <class F>
static int every_cut(uint64_t total, size_t words, const char* out_path, F&& range) {
  std::vector<int32_t> first, out;
  for (uint64_t c = 0; c <= total; ++c) {
    out.assign(words, -1);
    if (c > 0) range((uint64_t)0, c, out.data());
    if (c < total) range(c, total, out.data());
    if (c == 0) first = out;
    else if (out != first) { printf("cut %" PRIu64 " differs\n", c); return 1; }
  }
  printf("ok %" PRIu64 "\n", total + 1);
  return store(out_path, first);
}

static int cmd_runs(const char* runs_path, uint64_t H, int T, const char* out_path) {
  const std::vector<int32_t> runs = load<int32_t>(runs_path);
  const uint64_t n = runs.size() / 3;
  if (T > 0) {
    std::vector<int32_t> out(2 * H, -1);
    kmhg::expand_runs_host(runs.data(), n, H, out.data(), T);
    return store(out_path, out);
  }
  return every_cut(H, 2 * H, out_path, [&](uint64_t r0, uint64_t r1, int32_t* out) {
    kmhg::expand_runs_range(runs.data(), n, H, r0, r1, out);
  });
}

static int cmd_pairs(char** a, int T, const char* out_path) {
  const std::vector<uint32_t> pk = load<uint32_t>(a[0]);
  const std::vector<uint64_t> po = load<uint64_t>(a[1]);
  const std::vector<kmhg::RowInfo> ri = load<kmhg::RowInfo>(a[2]);
  const std::vector<int32_t> ps = load<int32_t>(a[3]);
  const uint64_t M = pk.size();
  if (!M || po.size() != M) { fprintf(stderr, "bad pair inputs\n"); return 2; }
  const uint64_t nl = ri[pk[M - 1]].x, P = po[M - 1] + nl * (nl - 1) / 2;
  if (T > 0) {
    std::vector<int32_t> out(3 * P, -1);
    kmhg::expand_pairs_host(pk.data(), po.data(), M, ri.data(), ps.data(), P, out.data(), T);
    return store(out_path, out);
  }
  return every_cut(P, 3 * P, out_path, [&](uint64_t r0, uint64_t r1, int32_t* out) {
    kmhg::expand_pairs_range(pk.data(), po.data(), M, ri.data(), ps.data(), r0, r1, out);
  });
}

static int cmd_pair_start(const char* path) {
  std::ifstream f(path);
  if (!f) { perror(path); return 2; }
  for (uint64_t n, t; f >> n >> t;) printf("%" PRIu64 "\n", kmhg::pair_start(n, t));
  return 0;
}

static int cmd_pool(int callers, int jobs, int max_tasks, bool fresh) {
  std::atomic<int> bad{0};
  std::vector<std::thread> th;
  for (int c = 0; c < callers; ++c)
    th.emplace_back([=, &bad] {
      uint64_t x = 77 + (uint64_t)c;
      for (int j = 0; j < jobs; ++j) {
        // 0 and 1 tasks first, then random counts up to max_tasks
        const int n = j < 2 ? std::min(j, max_tasks) : (int)(splitmix(x) % (uint64_t)(max_tasks + 1));
        std::atomic<int64_t> sum{0}, ran{0};
        kmhg::HostPool::get().run(n, [&](int i) { sum += i; ++ran; }, fresh);
        if (ran != n || sum != (int64_t)n * (n - 1) / 2) ++bad;
      }
    });
  for (auto& t : th) t.join();
  if (bad) printf("bad %d\n", bad.load());
  else printf("ok\n");
  return bad ? 1 : 0;
}

static int cmd_misc(int argc, char** argv) {
  for (int i = 2; i < argc; ++i) {
    const std::string a = argv[i];
    const size_t eq = a.find('=');
    if (eq == std::string::npos) return 2;
    const std::string name = a.substr(0, eq), v = a.substr(eq + 1);
    if (name == "span") {
      const size_t c = v.find(',');
      if (c == std::string::npos) return 2;
      const kmhg::Span s = kmhg::huge_span(
          reinterpret_cast<const void*>((uintptr_t)strtoull(v.c_str(), nullptr, 10)),
          (size_t)strtoull(v.c_str() + c + 1, nullptr, 10));
      printf("%" PRIu64 " %" PRIu64 "\n", (uint64_t)s.begin, (uint64_t)s.len);
    } else if (name == "class") {
      printf("%" PRIu64 "\n", (uint64_t)kmhg::pool_size_class((size_t)strtoull(v.c_str(), nullptr, 10)));
    } else if (name == "cap") {
      printf("%" PRIu64 "\n", kmhg::table_capacity(atoll(v.c_str())));
    } else if (name == "len") {
      std::vector<char> b(v.size() / 2);       // exact size: a scan past L is an ASan report
      for (size_t k = 0; k < b.size(); ++k) b[k] = (char)strtoul(v.substr(2 * k, 2).c_str(), nullptr, 16);
      printf("%zu\n", kmhg::effective_len(b.data(), b.size()));
    } else {
      return 2;
    }
  }
  return 0;
}

// ---------------------------------------------------------------------------- kmhg_pool.h
// The fake device's state, shared by the copies of FakeDev.  Every call is counted.  An event
// completes when the script says so; a wait for one that has not completed it (script: there
// is nobody else to do so), or blocks until complete_all() has (threads).
struct FakeState {
  std::mutex mu;
  std::condition_variable cv;
  bool blocking = false;
  std::map<void*, int> ids;            // the blocks handed out and not yet freed
  std::map<int, int> dev_of;           // by block id: the device it was allocated on
  std::vector<int> freed;              // ids in the order freed, negated if on another device
  std::vector<char> done{1};           // by event; [0] is not an event
  int next_id = 0;
  long allocs = 0, frees = 0, creates = 0, records = 0, ewaits = 0, swaits = 0, dones = 0;
  int fail_oom = 0, fail_error = 0, fail_event = 0, fail_record = 0;
  void complete_all() {
    std::lock_guard<std::mutex> g(mu);
    std::fill(done.begin(), done.end(), 1);
    cv.notify_all();
  }
};
struct FakeFailure { kmhg::PoolAlloc st; std::string text; };
struct FakeDev {
  FakeState* f;
  static inline thread_local int cur = 0;
  int current() { return cur; }
  void use(int dev) { cur = dev; }
  kmhg::PoolAlloc alloc(size_t sz, void** p, std::string* text) {
    std::lock_guard<std::mutex> g(f->mu);
    ++f->allocs;
    if (f->fail_oom > 0) { --f->fail_oom; return kmhg::PoolAlloc::oom; }
    if (f->fail_error > 0) { --f->fail_error; *text = "fake device error"; return kmhg::PoolAlloc::error; }
    *p = malloc(std::min<size_t>(sz, 64));
    f->ids[*p] = ++f->next_id;
    f->dev_of[f->next_id] = cur;
    return kmhg::PoolAlloc::ok;
  }
  void free(void* p) {
    std::lock_guard<std::mutex> g(f->mu);
    ++f->frees;
    auto it = f->ids.find(p);
    if (it != f->ids.end()) {
      f->freed.push_back(f->dev_of[it->second] == cur ? it->second : -it->second);
      f->ids.erase(it);
    }
    ::free(p);                          // a second free of p is ASan's to report
  }
  void* event() {
    std::lock_guard<std::mutex> g(f->mu);
    ++f->creates;
    if (f->fail_event > 0) { --f->fail_event; return nullptr; }
    f->done.push_back(0);
    return reinterpret_cast<void*>((uintptr_t)(f->done.size() - 1));
  }
  bool record(void* ev, void*) {
    std::lock_guard<std::mutex> g(f->mu);
    ++f->records;
    if (f->fail_record > 0) { --f->fail_record; return false; }
    f->done[(uintptr_t)ev] = 0;
    return true;
  }
  bool done(void* ev) {
    std::lock_guard<std::mutex> g(f->mu);
    ++f->dones;
    return f->done[(uintptr_t)ev] != 0;
  }
  void wait_event(void* ev) {
    std::unique_lock<std::mutex> g(f->mu);
    ++f->ewaits;
    if (f->blocking) f->cv.wait(g, [&] { return f->done[(uintptr_t)ev] != 0; });
    else f->done[(uintptr_t)ev] = 1;
  }
  void wait_stream(void*) {
    std::lock_guard<std::mutex> g(f->mu);
    ++f->swaits;
  }
  [[noreturn]] void alloc_failed(kmhg::PoolAlloc st, const std::string& text) {
    throw FakeFailure{st, text};
  }
};
using FakePool = kmhg::BlockPool<FakeDev>;
using FakeGroup = kmhg::ReleaseGroupT<FakeDev>;
struct FakeRec { void* ev; };
using FakeRecords = kmhg::RecordPool<FakeDev, FakeRec>;
// four records at a time, each with an event of the fake device's
static void fake_rec_grow(FakeDev d, std::vector<FakeRec>& out) {
  for (int i = 0; i < 4; ++i) out.push_back(FakeRec{d.event()});
}

// "ret=<r> allocs= frees= creates= records= ewaits= swaits= cached= idle= dev= live= free= pending=
// freed=": the backend's call counts, cached(), the idle events, the current device, and every
// block by state as <id>:<device>:<class> (pending ones with :<event>:<owns_ev>), sorted by id
static void pool_line(FakePool& pool, FakeState& f, const std::string& ret) {
  const FakePool::Snapshot s = pool.snapshot();
  std::lock_guard<std::mutex> g(f.mu);
  printf("ret=%s allocs=%ld frees=%ld creates=%ld records=%ld ewaits=%ld swaits=%ld cached=%zu"
         " idle=%zu dev=%d", ret.c_str(), f.allocs, f.frees, f.creates, f.records, f.ewaits,
         f.swaits, s.cached, s.idle_events, FakeDev::cur);
  const auto list = [&](const char* name, const std::vector<FakePool::Block>& v, bool ev) {
    std::vector<std::string> out;
    for (const auto& b : v) {
      char buf[96];
      int n = snprintf(buf, sizeof buf, "%06d:%d:%zu", f.ids.at(b.p), b.key.first, b.key.second);
      if (ev) snprintf(buf + n, sizeof buf - (size_t)n, ":%d:%d", (int)(uintptr_t)b.ev, b.owns_ev ? 1 : 0);
      out.push_back(buf);
    }
    std::sort(out.begin(), out.end());
    printf(" %s=", name);
    for (size_t i = 0; i < out.size(); ++i)    // (ids zero-padded for the sort, printed plain)
      printf("%s%s", i ? "," : "", out[i].c_str() + out[i].find_first_not_of('0'));
  };
  list("live", s.live, false);
  list("free", s.free, false);
  list("pending", s.pending, true);
  printf(" freed=");
  for (size_t i = 0; i < f.freed.size(); ++i) printf("%s%d", i ? "," : "", f.freed[i]);
  printf("\n");
}

static int cmd_block_pool(const char* path) {
  std::ifstream in(path);
  if (!in) { perror(path); return 2; }
  std::vector<std::vector<std::string>> ops;
  for (std::string line; std::getline(in, line);) {
    std::istringstream is(line);
    std::vector<std::string> a;
    for (std::string w; is >> w;) a.push_back(w);
    if (!a.empty()) ops.push_back(a);
  }
  kmhg::PoolKnobs kn;
  size_t at = 0;
  if (!ops.empty() && ops[0][0] == "knobs" && ops[0].size() == 3) {
    kn.depth = (size_t)atoi(ops[0][1].c_str());
    kn.best_fit = ops[0][2] != "0";
    at = 1;
  }
  FakeState f;
  FakePool pool(kn, FakeDev{&f});
  std::map<std::string, void*> names;
  std::vector<std::unique_ptr<FakeGroup>> groups;      // innermost last
  size_t ahead = kn.ahead;
  std::unique_ptr<FakeRecords> recs;
  std::map<std::string, FakeRec> rec_names;
  char unknown = 0;
  const auto stream = [](const std::string& w) { return reinterpret_cast<void*>((uintptr_t)atoi(w.c_str())); };
  for (; at < ops.size(); ++at) {
    const std::vector<std::string>& a = ops[at];
    const std::string& op = a[0];
    std::string ret = "-";
    if (op == "dev" && a.size() == 2) {
      FakeDev::cur = atoi(a[1].c_str());
    } else if (op == "alloc" && a.size() == 3) {
      try {
        void* p = pool.alloc((size_t)strtoull(a[2].c_str(), nullptr, 10));
        names[a[1]] = p;
        std::lock_guard<std::mutex> g(f.mu);
        ret = std::to_string(f.ids.at(p));
      } catch (const FakeFailure& e) {
        ret = e.st == kmhg::PoolAlloc::oom ? "oom" : "error:" + e.text;
        std::replace(ret.begin(), ret.end(), ' ', '_');
      }
    } else if (op == "alloc_on" && a.size() == 4) {
      void* p = pool.alloc((size_t)strtoull(a[2].c_str(), nullptr, 10), stream(a[3]));
      names[a[1]] = p;
      std::lock_guard<std::mutex> g(f.mu);
      ret = std::to_string(f.ids.at(p));
    } else if (op == "dones") {
      std::lock_guard<std::mutex> g(f.mu);
      ret = std::to_string(f.dones);
    } else if (op == "ahead" && a.size() == 2 && !recs) {
      ahead = (size_t)atoi(a[1].c_str());
    } else if (op == "rec_take" && a.size() == 2) {
      if (!recs) recs = std::make_unique<FakeRecords>(ahead, FakeDev{&f});
      const FakeRec r = recs->take([&](std::vector<FakeRec>& out) { fake_rec_grow(FakeDev{&f}, out); });
      rec_names[a[1]] = r;
      const auto n = recs->sizes();
      ret = std::to_string((uintptr_t)r.ev) + ":" + std::to_string(n.first) + ":" + std::to_string(n.second);
    } else if (op == "rec_give" && (a.size() == 2 || a.size() == 3) && recs) {
      const FakeRec r = rec_names.at(a[1]);
      if (a.size() == 3 && !FakeDev{&f}.record(r.ev, stream(a[2]))) return 2;
      recs->give(r, a.size() == 3);
    } else if (op == "release" && (a.size() == 2 || a.size() == 3)) {
      void* p = a[1] == "null" ? nullptr : a[1] == "unknown" ? (void*)&unknown : names.at(a[1]);
      if (a.size() == 3) pool.release(p, stream(a[2]), true);
      else pool.release(p);
    } else if (op == "group_begin" && a.size() == 2) {
      groups.push_back(std::make_unique<FakeGroup>(pool, stream(a[1])));
    } else if (op == "synced" && !groups.empty()) {
      groups.back()->synced = true;
    } else if (op == "group_end" && !groups.empty()) {
      groups.pop_back();
    } else if (op == "own_event" && a.size() == 2) {   // made and recorded by the caller, not the pool
      FakeDev d{&f};
      void* ev = d.event();
      if (!ev || !d.record(ev, stream(a[1]))) return 2;
      ret = std::to_string((uintptr_t)ev);
    } else if (op == "adopt" && a.size() == 2 && !groups.empty()) {
      groups.back()->adopt(reinterpret_cast<void*>((uintptr_t)atoi(a[1].c_str())));
    } else if (op == "complete" && a.size() == 2) {
      std::lock_guard<std::mutex> g(f.mu);
      f.done.at((size_t)atoi(a[1].c_str())) = 1;
    } else if (op == "fail" && a.size() == 3) {
      int* n = a[1] == "alloc-oom" ? &f.fail_oom : a[1] == "alloc-error" ? &f.fail_error
               : a[1] == "event" ? &f.fail_event : a[1] == "record" ? &f.fail_record : nullptr;
      if (!n) return 2;
      *n = atoi(a[2].c_str());
    } else if (op == "trim") {
      pool.trim();
    } else if (op == "cached") {
      ret = std::to_string(pool.cached());
    } else {
      fprintf(stderr, "bad pool operation: %s\n", op.c_str());
      return 2;
    }
    pool_line(pool, f, ret);
  }
  return 0;
}

static int cmd_block_pool_threads(int T, int nops, bool on_stream) {
  FakeState f;
  f.blocking = true;
  FakePool pool(kmhg::PoolKnobs{}, FakeDev{&f});
  FakeRecords recs(2, FakeDev{&f});
  std::atomic<bool> stop{false};
  std::atomic<int> bad{0};
  std::thread completer([&] {
    while (!stop) { f.complete_all(); std::this_thread::yield(); }
  });
  const size_t classes[3] = {200, 4096, (3u << 20) + 1};
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t] {
      uint64_t x = 1234 + (uint64_t)t;
      FakeDev::cur = t & 1;
      void* const s = reinterpret_cast<void*>((uintptr_t)(t + 1));
      void* const other = reinterpret_cast<void*>((uintptr_t)(T + 1));
      std::vector<char*> held;
      const auto take = [&] {         // a block is this thread's alone: its first byte says so
        const size_t sz = classes[splitmix(x) % 3];
        char* p = static_cast<char*>(on_stream && splitmix(x) % 4 ? pool.alloc(sz, s) : pool.alloc(sz));
        *p = (char)t;
        held.push_back(p);
      };
      const auto give = [&](void* stream, bool ordered) {
        if (held.empty()) return;
        const size_t i = splitmix(x) % held.size();
        if (*held[i] != (char)t) ++bad;
        pool.release(held[i], stream, ordered);
        held.erase(held.begin() + (long)i);
      };
      for (int i = 0; i < nops; ++i) {
        const uint64_t r = splitmix(x) % 8;
        if (held.size() >= 8 || r == 3) give(nullptr, false);
        else if (r < 3) take();
        else if (r < 6) give(s, true);
        else {                        // a group: a few of its stream's, one of another stream's
          FakeGroup rg(pool, s);
          take();
          for (int j = 0; j < 3; ++j) give(s, true);
          give(other, true);
          rg.synced = r == 7 && (i & 1);
          if (on_stream) {            // a build's record: freed unwaited every other time
            const FakeRec rec =
                recs.take([&](std::vector<FakeRec>& out) { fake_rec_grow(FakeDev{&f}, out); });
            const bool in_flight = (i & 2) && FakeDev{&f}.record(rec.ev, s);
            if (in_flight && !rg.synced) rg.adopt(rec.ev);
            recs.give(rec, in_flight);
          }
        }
      }
      while (!held.empty()) give(nullptr, false);
    });
  for (auto& t : th) t.join();
  stop = true;
  completer.join();
  f.complete_all();
  pool.trim();
  const FakePool::Snapshot s = pool.snapshot();
  const bool clean = s.live.empty() && s.free.empty() && s.pending.empty() && s.cached == 0 &&
                     f.ids.empty() && (long)f.freed.size() == f.next_id && !bad;
  printf("%s blocks=%d live=%zu free=%zu pending=%zu unfreed=%zu bad=%d\n", clean ? "ok" : "bad",
         f.next_id, s.live.size(), s.free.size(), s.pending.size(), f.ids.size(), bad.load());
  return clean ? 0 : 1;
}

// ---------------------------------------------------------------------------- kmhg_reads.h
// integers of argv[from ..), or of a comma-separated list, heap-allocated at their exact number
static std::vector<int32_t> ints_of(int argc, char** argv, int from) {
  std::vector<int32_t> v;
  for (int i = from; i < argc; ++i) v.push_back((int32_t)strtoll(argv[i], nullptr, 10));
  return v;
}
static std::vector<int32_t> ints_of(const char* csv) {
  std::vector<int32_t> v;
  std::istringstream is(csv);
  for (std::string w; std::getline(is, w, ',');) v.push_back((int32_t)strtoll(w.c_str(), nullptr, 10));
  return v;
}

static int cmd_read_call(int argc, char** argv) {
  const bool sh1 = std::string(argv[2]) == "sh1";
  const std::vector<int32_t> p = ints_of(argc, argv, 3);
  if (p.size() != (sh1 ? 6u : 8u)) return 2;
  const kmhg::ReadCall c = sh1 ? kmhg::read_call_sh1(p.data()) : kmhg::read_call_rp(p.data());
  if (c.err) { printf("err=%d msg=%s\n", c.err, c.msg); return 0; }
  printf("err=0 k=%d sources=%u single=%d sh1=%d min_ll=%.17g mq=%d source=%u max_reads=%" PRIu64
         "\n", c.k, c.sources, c.single ? 1 : 0, c.walk.sh1 ? 1 : 0, c.walk.min_ll, c.walk.mq,
         c.walk.source, c.max_reads);
  return 0;
}

static int cmd_read_batches(uint64_t span_max, const char* path) {
  std::ifstream f(path);
  if (!f) { perror(path); return 2; }
  std::vector<int64_t> off{0};
  for (int64_t l; f >> l;) off.push_back(off.back() + l);
  off.shrink_to_fit();
  std::vector<std::pair<size_t, size_t>> out;
  const kmhg::Refusal bad = kmhg::read_batches(off.data(), off.size() - 1, span_max, out);
  if (bad.err) printf("err=%d msg=%s\n", bad.err, bad.msg);
  for (auto& b : out) printf("%zu %zu\n", b.first, b.second);
  return 0;
}

static void print_reads(const kmhg::ReadsHost& r) {
  printf("n=%zu off=", r.n());
  for (size_t i = 0; i < r.off.size(); ++i) printf("%s%" PRId64, i ? "," : "", r.off[i]);
  printf(" hasq=");
  for (uint8_t h : r.hasq) printf("%d", h);
  printf(" seq=%016" PRIx64 " qual=%016" PRIx64 "\n", fnv(r.seq.data(), r.seq.size()),
         fnv(r.qual.data(), r.qual.size()));
}

static int cmd_reads_longer(int k, const char* path) {
  kmhg::ReadsHost r, keep;
  kmhg::read_fastx(path, UINT64_MAX, 0, r, nullptr);
  const kmhg::ReadsHost* use = kmhg::reads_longer_than(r, k, keep);
  printf("same=%d ", use == &r ? 1 : 0);
  print_reads(*use);
  return 0;
}

static int cmd_read_fastx(const char* path, int k, uint64_t max_reads, size_t batch) {
  kmhg::ReadsHost r;
  std::vector<int64_t> lens;
  std::string hasq;
  uint64_t hs = fnv(nullptr, 0), hq = hs;
  const auto take = [&](kmhg::ReadsHost& b) {
    for (size_t i = 0; i < b.n(); ++i) {
      lens.push_back(b.off[i + 1] - b.off[i]);
      hasq.push_back(b.hasq[i] ? '1' : '0');
    }
    hs = fnv(b.seq.data(), b.seq.size(), hs);
    hq = fnv(b.qual.data(), b.qual.size(), hq);
  };
  const int64_t read_n = kmhg::read_fastx(path, max_reads, k, r, [&](kmhg::ReadsHost& b) {
    printf("B %zu %zu\n", b.n(), b.seq.size());
    take(b);
  }, batch);
  take(r);
  printf("T read_n=%" PRId64 " records=%" PRId64 " lens=", read_n, r.records);
  for (size_t i = 0; i < lens.size(); ++i) printf("%s%" PRId64, i ? "," : "", lens[i]);
  printf(" hasq=%s seq=%016" PRIx64 " qual=%016" PRIx64 "\n", hasq.c_str(), hs, hq);
  return 0;
}

static int cmd_spectrum_status(uint32_t S, const char* comb_csv, const char* inner_csv) {
  const std::vector<int32_t> comb = ints_of(comb_csv), inner = ints_of(inner_csv);
  if (comb.size() != inner.size()) return 2;
  printf("%d\n", kmhg::spectrum_status(comb.data(), inner.data(), (int)comb.size(), S));
  return 0;
}

// ---------------------------------------------------------------------------- kmhg_querycall.h
static long long ll(const char* s) { return strtoll(s, nullptr, 10); }

static int cmd_query(int argc, char** argv) {
  using namespace kmhg;
  const std::string m = argv[2];
  if (m == "call" && (argc == 5 || argc == 7)) {
    const size_t L = (size_t)strtoull(argv[3], nullptr, 10);
    const QueryCall c = argc == 5 ? query_call(L, atoi(argv[4]))
                                  : query_call_range(L, atoi(argv[4]), ll(argv[5]), ll(argv[6]));
    const QueryCall f = c.of_part().as_runs().on_rc();       // the modes keep call and refusal
    if (f.code != c.code || f.text != c.text || f.w0 != c.w0 || f.w1 != c.w1 || !f.part ||
        !f.runs || !f.rc)
      return 1;
    if (c.code) printf("err=%d msg=%s\n", c.code, c.text);
    else
      printf("err=0 L=%" PRId64 " k=%d w0=%" PRId64 " w1=%" PRId64 " part=%d runs=%d rc=%d\n", c.L,
             c.k, c.w0, c.w1, c.part ? 1 : 0, c.runs ? 1 : 0, c.rc ? 1 : 0);
    return 0;
  }
  if (m == "rules") {
    for (int i = 3; i < argc; ++i) {
      std::vector<long long> v;
      const char* eq = strchr(argv[i], '=');
      if (!eq) return 2;
      std::istringstream is(eq + 1);
      for (std::string w; std::getline(is, w, ',');) v.push_back(ll(w.c_str()));
      const std::string name(argv[i], (size_t)(eq - argv[i]));
      if (name == "guess" && v.size() == 1)
        printf("guess=%" PRIu64 "\n", query_rows_guess(v[0]));
      else if (name == "runs_pay" && v.size() == 2)
        printf("runs_pay=%d\n", runs_pay((uint64_t)v[0], (uint64_t)v[1]) ? 1 : 0);
      else if (name == "redo" && v.size() == 2)
        printf("redo=%d\n", needs_exact_redo((uint64_t)v[0], (uint64_t)v[1]) ? 1 : 0);
      else if (name == "diag" && v.size() == 7)
        printf("diag=%d\n", diag_eligible((int)v[0], (int)v[1], (uint32_t)v[2], v[3], (uint64_t)v[4],
                                          v[5] != 0, v[6] != 0) ? 1 : 0);
      else
        return 2;
    }
    return 0;
  }
  if (m == "devices" && argc == 5) {
    std::vector<int> out;
    const DeviceList bad = parse_device_list(argv[3], atoi(argv[4]), out);
    if (bad.code) { printf("err=%d msg=%s\n", bad.code, bad.text.c_str()); return 0; }
    printf("err=0 devices=");
    for (size_t i = 0; i < out.size(); ++i) printf("%s%d", i ? "," : "", out[i]);
    printf("\n");
    return 0;
  }
  if (m == "shards" && argc == 6) {
    const int64_t L = ll(argv[3]);
    const int k = atoi(argv[4]), G = atoi(argv[5]);
    for (int i = 0; i < G; ++i) {
      const Span64 w = shard_windows(L - k + 1, i, G);
      const Span64 c = shard_chars(L, k, w.begin, w.end);
      printf("w0=%" PRId64 " w1=%" PRId64 " c0=%" PRId64 " c1=%" PRId64 "\n", w.begin, w.end,
             c.begin, c.end);
    }
    return 0;
  }
  if (m == "offsets" && argc == 4) {
    std::vector<int64_t> H, off;
    std::istringstream is(argv[3]);
    for (std::string w; std::getline(is, w, ',');) H.push_back(ll(w.c_str()));
    const int64_t total = part_offsets(H, off);
    printf("total=%" PRId64 " off=", total);
    for (size_t i = 0; i < off.size(); ++i) printf("%s%" PRId64, i ? "," : "", off[i]);
    printf("\n");
    return 0;
  }
  return 2;
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: see the file header\n"); return 2; }
  const std::string c = argv[1];
  if (c == "plan") return cmd_plan(argc, argv);
  if (c == "misc") return cmd_misc(argc, argv);
  if (c == "query") return cmd_query(argc, argv);
  if (c == "stripes" && argc == 5)
    return cmd_stripes(strtoull(argv[2], nullptr, 10), atoi(argv[3]), strtoull(argv[4], nullptr, 10));
  if (c == "runs" && argc == 6 && atoi(argv[4]) > 0)
    return cmd_runs(argv[2], strtoull(argv[3], nullptr, 10), atoi(argv[4]), argv[5]);
  if (c == "runs-split" && argc == 5)
    return cmd_runs(argv[2], strtoull(argv[3], nullptr, 10), 0, argv[4]);
  if (c == "pairs" && argc == 8 && atoi(argv[6]) > 0) return cmd_pairs(argv + 2, atoi(argv[6]), argv[7]);
  if (c == "pairs-split" && argc == 7) return cmd_pairs(argv + 2, 0, argv[6]);
  if (c == "pair-start" && argc == 3) return cmd_pair_start(argv[2]);
  if (c == "pool" && argc == 3) return cmd_block_pool(argv[2]);
  if (c == "pool" && argc == 5 && std::string(argv[2]) == "threads")
    return cmd_block_pool_threads(atoi(argv[3]), atoi(argv[4]), false);
  if (c == "pool" && argc == 5 && std::string(argv[2]) == "stream-threads")
    return cmd_block_pool_threads(atoi(argv[3]), atoi(argv[4]), true);
  if (c == "pool" && argc == 6)
    return cmd_pool(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]) != 0);
  if (c == "read-call" && argc >= 4) return cmd_read_call(argc, argv);
  if (c == "read-batches" && argc == 4) return cmd_read_batches(strtoull(argv[2], nullptr, 10), argv[3]);
  if (c == "reads-longer" && argc == 4) return cmd_reads_longer(atoi(argv[2]), argv[3]);
  if (c == "read-fastx" && argc == 6)
    return cmd_read_fastx(argv[2], atoi(argv[3]), strtoull(argv[4], nullptr, 10),
                          (size_t)strtoull(argv[5], nullptr, 10));
  if (c == "spectrum-status" && argc == 5)
    return cmd_spectrum_status((uint32_t)atoi(argv[2]), argv[3], argv[4]);
  if (c == "fastx" && argc == 4) return cmd_fastx(argv[2], atol(argv[3]));
  if (c == "khash" && argc == 4) return cmd_khash(atol(argv[2]), strtoull(argv[3], nullptr, 10));
  if (c == "index" && argc == 4) return cmd_index(argv[2], atoi(argv[3]));
  if (c == "reads" && argc == 5) return cmd_reads(argv[2], atoi(argv[3]), atoi(argv[4]));
  fprintf(stderr, "bad arguments\n");
  return 2;
}
