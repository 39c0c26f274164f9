// kmhg_querycall.h -- the host side of seq.kmer.pos queries (host only: no HIP, any C++17 compiler).
//
// What the query entries decide before and between their HIP calls: the description of one query
// as data (QueryCall: length, k, window range and the named modes, or a refusal with the entries'
// code and text), the rules of the launch sequence (query_rows_guess, runs_pay, needs_exact_redo,
// diag_eligible), the KMHG_DEVICES grammar (parse_device_list), the multi-device split and the
// chars a window range reads (shard_windows, shard_chars) and the parts' row offsets
// (part_offsets), and the occurrence cap (kmhg_set_max_occ): its argument rule (max_occ_refusal)
// and the rule of one window record under it (qrec_kept, qrec_rows), which k_qrec_mask of
// kmhg_kernels.hip evaluates per window -- the rule exists once.  A refusal is a value; nothing
// here throws on a bad argument or reads the environment.  The engine keeps every HIP call,
// every lock and the two lookups (the KMHG_DEVICES text and the device count).
// tools/asan/host_check runs all of it under ASan + UBSan (tests/test_query_host.py), and
// tools/asan/maxocc_check the occurrence cap's rules (tests/test_maxocc_host.py).
//
// KMHG_DEVICES routes kmhg_query_run alone.  kmhg_query_run_rc does not look at it and runs on
// the index's own device, like every device-pointer entry.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/kmhgpu.h"
#include "kmhg_common.h"

// (hidden: nothing of this header joins the library's dynamic symbols)
#pragma GCC visibility push(hidden)
namespace kmhg {

// One query, whole: the engine's query_device looks at nothing else.
struct QueryCall {
  int code = KMHG_OK;          // a refusal: the engine's fail(code, text)
  const char* text = nullptr;
  int64_t L = 0;               // chars of the query sequence
  int k = 0;
  int64_t w0 = 0, w1 = 0;      // windows [w0, w1) of its L - k + 1
  bool part = false;           // over a part of an owner-computes build: keeps its tile offsets
  bool runs = false;           // rows as diagonal runs where that is smaller (runs_pay)
  bool rc = false;             // the reverse strand: w0, w1 and the rows' i in rc(seq)'s coordinates
  int64_t max_occ = 0;         // the index's occurrence cap when the entry was called; 0: none
  int sampling = 1;            // the index's minimizer w where the query is at the index's k; 1: none
  QueryCall of_part() const { QueryCall c = *this; c.part = true; return c; }
  QueryCall as_runs() const { QueryCall c = *this; c.runs = true; return c; }
  QueryCall on_rc(bool on = true) const { QueryCall c = *this; c.rc = on; return c; }
  QueryCall with_max_occ(int64_t n) const { QueryCall c = *this; c.max_occ = n; return c; }
  QueryCall with_sampling(int w) const { QueryCall c = *this; c.sampling = w; return c; }
};

inline QueryCall query_refusal(int code, const char* text) {
  QueryCall c;
  c.code = code;
  c.text = text;
  return c;
}

// Every window of a sequence of L chars (sequence_kmer_positions, src/kmer_hash.c:1163-1164: its
// one sentence first, then the int positions' limit).
inline QueryCall query_call(size_t L, int k) {
  if ((int64_t)L <= k || k > 31 || k < 1)
    return query_refusal(KMHG_EINVAL,
                         "the sequence should be longer than k and k should not be longer than 31");
  if (L >= (size_t)INT32_MAX)
    return query_refusal(KMHG_EOVERFLOW, "sequence longer than 2^31-1 (int positions)");
  QueryCall c;
  c.L = (int64_t)L;
  c.k = k;
  c.w1 = (int64_t)L - k + 1;
  return c;
}

// Windows [w_begin, w_end) of it (an empty range is a query without rows).
inline QueryCall query_call_range(size_t L, int k, int64_t w_begin, int64_t w_end) {
  QueryCall c = query_call(L, k);
  if (c.code != KMHG_OK) return c;
  if (w_begin < 0 || w_end > c.w1 || w_begin > w_end)
    return query_refusal(KMHG_EINVAL, "window range out of bounds");
  c.w0 = w_begin;
  c.w1 = w_end;
  return c;
}

// kmhg_set_max_occ's argument: 0 (off) or a cap of 1 .. 2^31-1 occurrences.
inline QueryCall max_occ_refusal(int64_t n) {
  if (n < 0 || n > (int64_t)INT32_MAX)
    return query_refusal(KMHG_EINVAL, "max.occ must be between 0 and 2^31-1");
  return QueryCall{};
}

// One window record under a cap of max_occ >= 1 occurrences.  `rec` is the window's qrec word
// (put_qrec of kmhg_kernels.hip): 0 for no hit, the one hit's position, or QREC_MAXOCC_MULTI,
// and only then `count` (qmulti's .x, >= 2) is looked at.  A window whose k-mer occurs more than
// max_occ times in the index is dropped whole; one with exactly max_occ keeps every hit.
constexpr uint32_t QREC_MAXOCC_MULTI = 0x80000000u;   // QREC_MULTI of kmhg_kernels.hip
__host__ __device__ constexpr bool qrec_kept(uint32_t rec, uint32_t count, uint32_t max_occ) {
  return rec != QREC_MAXOCC_MULTI || count <= max_occ;
}
// What the window adds to its tile's hit total: 0, 1 or its count.
__host__ __device__ constexpr uint32_t qrec_rows(uint32_t rec, uint32_t count, uint32_t max_occ) {
  return rec == 0 ? 0u : rec != QREC_MAXOCC_MULTI ? 1u : count <= max_occ ? count : 0u;
}

// Rows are written into a guessed capacity before their number is known (no host round trip
// inside the query): one per window, an eighth more, and 64.
inline uint64_t query_rows_guess(int64_t Nw) { return (uint64_t)Nw + ((uint64_t)Nw >> 3) + 64; }

// A runs query keeps its H rows as NR diagonal runs only where they are smaller: 12 B per run
// against 8 B per row.
inline bool runs_pay(uint64_t H, uint64_t NR) { return H && 3 * NR < 2 * H; }

// More rows than the buffer they were emitted into holds -- heavy repeats: emitted again into
// an exact one.
inline bool needs_exact_redo(uint64_t H, uint64_t cap) { return H > cap; }

// The diagonal path (k_query_probe) serves a position index (no sources) queried at its own k
// that has windows, keys and the build's code words; `knob`: KMHG_QUERY_DIAG is not 0 (test build).
// Never a sampled index (sampling > 1, kmhg_minimizer.h): the path predicts a hit at the index
// window after a verified one, which holds only where every valid window is in the index.
inline bool diag_eligible(int kq, int index_k, uint32_t sources, int64_t index_windows, uint64_t U,
                          bool has_codes, bool knob, int sampling = 1) {
  return knob && kq == index_k && sources == 0 && index_windows > 0 && U > 0 && has_codes &&
         sampling <= 1;
}

struct DeviceList {
  int code = KMHG_OK;          // a refusal, as QueryCall's
  std::string text;
};

// KMHG_DEVICES: device ordinals below n_devices separated by commas, repeats and order kept (a
// device listed twice runs two parts).  The empty text lists nothing.
inline DeviceList parse_device_list(const std::string& str, int n_devices, std::vector<int>& out) {
  if (str.empty()) return {};
  size_t a = 0;
  while (a <= str.size()) {
    size_t b = str.find(',', a);
    if (b == std::string::npos) b = str.size();
    const std::string tok = str.substr(a, b - a);
    char* end = nullptr;
    const long d = std::strtol(tok.c_str(), &end, 10);
    if (tok.empty() || *end || d < 0 || d >= n_devices) {
      out.clear();
      return {KMHG_EINVAL, "KMHG_DEVICES must list device ordinals (0.." +
                               std::to_string(n_devices - 1) + "), got \"" + str + "\""};
    }
    out.push_back((int)d);
    a = b + 1;
  }
  return {};
}

struct Span64 {
  int64_t begin = 0, end = 0;
};

// Part i of G of a multi-device query: contiguous window ranges covering [0, Nw).  (The
// remainder goes to the later parts here and to the first ranks in dist.py's shard_ranges: two
// callers, each with its own split, and rows that concatenate to the same result under either.)
inline Span64 shard_windows(int64_t Nw, int i, int G) {
  return {Nw * i / G, Nw * (i + 1) / G};
}

// The chars [begin, end) of a sequence of L that a query of windows [w0, w1) may read: the
// window rule needs [w0 - 1, w1 + k - 1) (the N before a window, the end-drop test); the tile
// stage's aligned loads and halo read a few more around them, which feed only windows outside
// the range.  An empty range reads nothing.  dist.py's slice_bounds is the same rule for a rank
// without the library; tests/test_query_host.py holds the two together.
inline Span64 shard_chars(int64_t L, int k, int64_t w0, int64_t w1) {
  if (w1 <= w0) return {};
  return {std::max<int64_t>(0, (w0 & ~15ll) - 64), std::min<int64_t>(L, w1 + k + 64)};
}

// Part i's rows start at row off[i] of the whole result; returns the total.
inline int64_t part_offsets(const std::vector<int64_t>& H, std::vector<int64_t>& off) {
  int64_t at = 0;
  off.clear();
  for (int64_t h : H) {
    off.push_back(at);
    at += h;
  }
  return at;
}

}  // namespace kmhg
#pragma GCC visibility pop
