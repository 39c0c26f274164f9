// kmhg_reads.h -- the host side of read counting (host only: no HIP, any C++17 compiler).
//
// What count.kmers.fq.sh.rp, count.kmers.fq.sh and the two spectra do before anything reaches the
// device: the decoding of a call's int32 parameter vector (ReadCall), the packed host reads and
// the file reader's loop (ReadsHost, read_fastx, reads_longer_than), the split of packed reads
// into device batches (read_batches, batch_span_ok), the quality table's formula (qll_host) and
// the spectrum's argument scan (spectrum_status).  A refusal is a value ({err, msg}: the engine's
// fail(err, msg)); nothing here throws on a bad argument or reads the environment.
// tools/asan/host_check runs all of it under ASan + UBSan (tests/test_reads_host.py).
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "kmhg_common.h"
#include "kmhg_fastx.h"
#include "../../include/kmhgpu.h"

// (hidden: nothing of this header joins the library's dynamic symbols)
#pragma GCC visibility push(hidden)
namespace kmhg {

// q_to_ll (src/Q_to_log_likelihood.h): -708 below '"', else log(1 - 10^(-(q-33)/10)) printed
// to 15 significant digits -- exactly the doubles the reference's table holds (checked against
// it by tests/golden/make_sh_golden.py).  The device table is this function at q = 0 .. 255.
inline double qll_host(int q) {
  if (q < 34) return -708.0;
  char buf[64];
  snprintf(buf, sizeof buf, "%.15g", std::log(1.0 - std::pow(10.0, -(double)(q - 33) / 10.0)));
  return std::strtod(buf, nullptr);
}

// Which of the reference's two read walks a batch is counted with: count.kmers.fq.sh.rp's
// log-likelihood iterator (min_ll) or count.kmers.fq.sh's character threshold (sh1, mq).
struct ReadWalk {
  bool sh1 = false;
  double min_ll = 0;
  int mq = 0;
  uint32_t source = 0;
};

struct Refusal {
  int err = KMHG_OK;
  const char* msg = nullptr;
};

// One read-counting call, decoded from its parameter vector: the engine looks at nothing else.
struct ReadCall {
  int err = KMHG_OK;           // a refusal: the engine's fail(err, msg)
  const char* msg = nullptr;
  int k = 0;
  uint32_t sources = 0;        // counts per k-mer of a suffix hash the call makes
  bool single = false;         // count.kmers.fq.sh: the single suffix_hash (info.kind = 3)
  ReadWalk walk;
  uint64_t max_reads = 0;      // records the file entries read at most
};

// count_kmers_fastq_sh_rp (src/kmer_hash.c:810-857): argument checks in the reference's order
// and with its texts; the remaining deviations are undefined-behaviour paths of the reference.
// p = (k, prefix_bits, min_q, thread_n, max_reads, max_mem, source_n, source).
inline ReadCall read_call_rp(const int32_t p[8]) {
  const int k = p[0];
  const uint32_t source_n = (uint32_t)p[6], source_i = (uint32_t)p[7];
  if (k < 1 || k > 32) return {KMHG_EINVAL, "k must be a positive integer less than 1+MAX_K"};
  if (source_n > 4 || source_n < 1) return {KMHG_EINVAL, "Source_n must be in the range 1 - 4"};
  if (source_i >= source_n) return {KMHG_EINVAL, "source_i must be less than source_n"};
  // k = 32: the reference's (1 << 2k) - 1 masks shift by 64 (undefined); prefix_bits > 2k with
  // k < 16 makes its suffix/prefix split underflow (src/kmer_reader.c:84-92)
  if (k == 32) return {KMHG_EINVAL, "k must be at most 31 for the suffix hash"};
  uint32_t pb = (uint32_t)p[1];
  if (pb > 36) pb = 36;
  if (2 * (uint32_t)k < 32 && pb > 2 * (uint32_t)k)
    return {KMHG_EINVAL, "prefix_bits must not exceed 2k"};
  ReadCall c;
  c.k = k;
  c.sources = source_n;
  c.walk = ReadWalk{false, qll_host((unsigned char)('!' + (unsigned char)p[2])), 0, source_i};
  c.max_reads = (uint64_t)(int64_t)p[4];   // (size_t) of an int
  return c;
}

// count_kmers_fastq_sh (src/kmer_hash.c:715-806); the deviations on the reference's undefined
// paths are listed in kmhgpu.h.
// p = (k, report_n, prefix_bits, max_memory, min_quality, max_read_n).
inline ReadCall read_call_sh1(const int32_t p[6]) {
  const int k = p[0];
  if (k < 1 || k > 32) return {KMHG_EINVAL, "k must be a positive integer less than 1+MAX_K"};
  if (k == 32) return {KMHG_EINVAL, "k must be at most 31 for the suffix hash"};
  const uint32_t prefix_bits = (uint32_t)p[2];
  const uint32_t suffix_bits = 2 * (uint32_t)k - prefix_bits;      // wraps when negative
  if (suffix_bits > 32) return {KMHG_EINVAL, "suffix bits (2k - prefix_bits) must be in 0 .. 32"};
  const uint64_t max_memory = (1ull << 30) * (uint64_t)(int64_t)p[3];
  if (prefix_bits > 60 || (8ull << prefix_bits) > max_memory)
    return {KMHG_EINVAL, "max_memory is too small for the prefix array of the suffix hash"};
  ReadCall c;
  c.k = k;
  c.sources = 1;
  c.single = true;
  // char min_quality = (char)params[4] + '!', compared as C char (the sum taken in unsigned, so
  // that no min_quality overflows it)
  c.walk = ReadWalk{true, 0.0, (int)(int8_t)(uint8_t)((uint32_t)p[4] + '!'), 0u};
  c.max_reads = (uint64_t)(int64_t)p[5];   // (size_t) of an int
  return c;
}

// Host reads packed for the GPU: bases and qualities concatenated, read r = [off[r], off[r+1]).
struct ReadsHost {
  std::vector<uint8_t> seq, qual, hasq;
  std::vector<int64_t> off{0};
  int64_t records = 0;                           // records consumed, short ones included
  void clear() { seq.clear(); qual.clear(); hasq.clear(); off.assign(1, 0); }
  void add(const std::string& sq, const std::string& ql, bool hq) {
    seq.insert(seq.end(), sq.begin(), sq.end());
    if (hq) qual.insert(qual.end(), ql.begin(), ql.end());
    else qual.resize(seq.size(), 0);
    hasq.push_back(hq ? 1 : 0);
    off.push_back((int64_t)seq.size());
  }
  size_t n() const { return hasq.size(); }
};

// Largest base span of one device batch: every per-read window bound is <= its read length, so
// their u32 sum cannot wrap below this.
constexpr uint64_t SH_SPAN_MAX = (uint64_t)UINT32_MAX;

// The device batches of n packed reads with offsets off[0 .. n]: ranges [i0, i1) of reads, taken
// greedily, each of fewer than span_max bases (offsets stay absolute, so a batch is a sub-range
// of the reads).  Refused before any range is emitted: a failing call counts nothing.
inline Refusal read_batches(const int64_t* off, size_t n, uint64_t span_max,
                            std::vector<std::pair<size_t, size_t>>& out) {
  if (!n) return {};
  if (n >= (size_t)UINT32_MAX) return {KMHG_EOVERFLOW, "more than 2^32-1 reads in one batch"};
  for (size_t i = 0; i < n; ++i)
    if ((uint64_t)(off[i + 1] - off[i]) >= span_max)
      return {KMHG_EOVERFLOW, "a read of 2^32 or more bases"};
  for (size_t i0 = 0; i0 < n;) {
    size_t i1 = i0 + 1;
    while (i1 < n && (uint64_t)(off[i1 + 1] - off[i0]) < span_max) ++i1;
    out.push_back({i0, i1});
    i0 = i1;
  }
  return {};
}

// A caller's device batch: its first and last offset must span fewer than SH_SPAN_MAX bases (a
// batch spanning 2^32 or more could wrap the u32 sum of its per-read window bounds).
inline bool batch_span_ok(int64_t first, int64_t last) {
  return last >= first && (uint64_t)last - (uint64_t)first < SH_SPAN_MAX;
}

// kmer_reader_read's loop (src/kmer_reader.c:51-73): records up to max_reads, those longer
// than k kept, qualities used when the record has them.  Batches of SH_BATCH bases.
constexpr size_t SH_BATCH = (size_t)256 << 20;

inline int64_t read_fastx(const char* path, uint64_t max_reads, int k, ReadsHost& r,
                          const std::function<void(ReadsHost&)>& flush,
                          size_t batch = SH_BATCH) {
  FastxReader rd(path);
  if (!rd.ok()) {   // gzopen failed: the reference's reader then reads nothing
    fprintf(stderr, "kmhg: unable to open %s: nothing counted\n", path);
    return 0;
  }
  std::string sq, ql;
  bool hq = false;
  uint64_t read_n = 0;
  int l;
  while ((l = rd.read(sq, ql, hq)) >= 0 && read_n < max_reads) {
    ++read_n;
    ++r.records;
    if (l <= k) continue;
    r.add(sq, ql, hq);
    if (r.seq.size() >= batch && flush) { flush(r); r.clear(); }
  }
  return (int64_t)read_n;
}

// The reads of r longer than k (r itself when all are): reads no longer than k were dropped
// when r was read with a smaller k.
inline const ReadsHost* reads_longer_than(const ReadsHost& r, int k, ReadsHost& keep) {
  bool all_long = true;
  for (size_t i = 0; i < r.n() && all_long; ++i) all_long = r.off[i + 1] - r.off[i] > k;
  if (all_long) return &r;
  for (size_t i = 0; i < r.n(); ++i) {
    const int64_t a = r.off[i], b = r.off[i + 1];
    if (b - a <= k) continue;
    keep.add(std::string((const char*)r.seq.data() + a, (size_t)(b - a)),
             std::string((const char*)r.qual.data() + a, (size_t)(b - a)), r.hasq[i] != 0);
  }
  return &keep;
}

// sh_count_spectrum_nc's argument scan (src/suffix_hash.c:338-421) over a hash of S counts per
// k-mer: 1, or the reference's code of the first offender: -3 (comb_inner not 0/1), -4
// (comb >= 2^S).
inline int spectrum_status(const int32_t* comb, const int32_t* comb_inner, int comb_n,
                           uint32_t S) {
  for (int i = 0; i < comb_n; ++i) {
    if ((uint32_t)comb_inner[i] > 1) return -3;
    if ((uint32_t)comb[i] >= (1u << S)) return -4;
  }
  return 1;
}

}  // namespace kmhg
#pragma GCC visibility pop
