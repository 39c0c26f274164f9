// kmhg_readsq.h -- the host side of reads.kmer.pos / reads.kmer.vote (no HIP: any C++17 compiler;
// the kernels of kmhg_readsq.hip include the same functions, so every rule exists once).
//
// reads.kmer.pos queries a batch of packed reads (seq = the bases of all reads, off[n + 1] their
// offsets) against a position index on both strands: rows (read, strand, i, j), read r's forward
// rows those of seq.kmer.pos(read_r), its reverse rows those of seq.kmer.pos.rc(read_r).
//
// The work is laid out as one VIRTUAL WINDOW SPACE of ns * n_bases entries (ns = 1 for one strand,
// 2 for both): read r owns entries [ns * off[r], ns * off[r + 1]), first its len forward window
// starts 0 .. len - 1, then (ns = 2) its len reverse window starts, each in the strand's own i
// order.  An entry whose window does not exist (the last k - 1 starts of a strand, an N, the
// dropped end window) holds an empty record.  Entry order is then row order -- read, forward
// before reverse, i -- so one record array (put_qrec's format) and one scan of its tile totals
// place every row, and an entry maps back to (read, strand, window) by a search in off alone.
//
// Here: the call as data (ReadsCall: the argument rules and refusals), the offsets' rule (one
// entry at a time, as the device evaluates it, and the host's loop over it), the entry -> (read,
// strand, window) map, the window rule of one read on either strand (the reference's walk with
// the read as the whole sequence, SURVEY.md §8.0: the mirrored end-drop is the rule of rc(read)
// read from the forward bases), the row-capacity guess and the rows' byte arithmetic, and the
// vote's cell, key and winner packing.  A refusal is a value; nothing here throws.
// tools/asan/readsq_check runs all of it under ASan + UBSan (tests/test_readsq_host.py).
#pragma once
#include <stdint.h>

#include "../../include/kmhgpu.h"
#include "kmhg_common.h"

// (hidden: nothing of this header joins the library's dynamic symbols)
#pragma GCC visibility push(hidden)
namespace kmhg {

constexpr int64_t RQ_MAX_BASES = (int64_t)INT32_MAX - 1;   // 2^31 - 2: i = window end fits an int
constexpr int64_t RQ_MAX_READS = (int64_t)INT32_MAX;       // the read column is an int

// One batched query, whole.
struct ReadsCall {
  int code = KMHG_OK;          // a refusal: the engine's fail(code, text)
  const char* text = nullptr;
  int64_t n_reads = 0, n_bases = 0;
  int k = 0;
  int ns = 0;                  // strands queried: 1 or 2
  bool rev_only = false;       // ns == 1: the reverse strand
  int64_t max_occ = 0;         // the index's occurrence cap when the entry was called; 0: none
  ReadsCall with_max_occ(int64_t n) const { ReadsCall c = *this; c.max_occ = n; return c; }
};

inline ReadsCall reads_refusal(int code, const char* text) {
  ReadsCall c;
  c.code = code;
  c.text = text;
  return c;
}

constexpr const char* RQ_OFF_TEXT =
    "read offsets must be non-decreasing from 0 to the number of bases";

// strands: 1 forward, 2 reverse, 3 both.  index_sources / index_k / index_sampling: what the
// index is (a counts index has sources; a minimizer-sampled one w > 1).
inline ReadsCall reads_call(int64_t n_bases, int64_t n_reads, int k, int strands,
                            uint32_t index_sources, int index_k, int index_sampling) {
  if (k < 1 || k > 31) return reads_refusal(KMHG_EINVAL, "k should be between 1 and 31");
  if (strands < 1 || strands > 3)
    return reads_refusal(KMHG_EINVAL, "strands must be 1 (forward), 2 (reverse) or 3 (both)");
  if (n_reads < 0 || n_bases < 0) return reads_refusal(KMHG_EINVAL, "negative read or base count");
  // bases that no read holds: off[0] = 0 cannot be n_bases.  Known before any launch, and the
  // kernels' searches need a read to stay inside off[0 .. n_reads] (a tile has entries only then)
  if (n_reads == 0 && n_bases > 0) return reads_refusal(KMHG_EINVAL, RQ_OFF_TEXT);
  if (index_sources)
    return reads_refusal(KMHG_EINVAL, "reads are queried against a position index, not a counts index");
  if (index_sampling > 1 && k == index_k)
    return reads_refusal(KMHG_EINVAL,
                         "a minimizer-sampled index is not queried with reads at its own k yet "
                         "(per-read minimizer selection is a follow-up)");
  if (n_bases > RQ_MAX_BASES)
    return reads_refusal(KMHG_EOVERFLOW, "more than 2^31-2 bases in one call: split the reads");
  if (n_reads > RQ_MAX_READS)
    return reads_refusal(KMHG_EOVERFLOW, "more than 2^31-1 reads in one call: split the reads");
  ReadsCall c;
  c.n_reads = n_reads;
  c.n_bases = n_bases;
  c.k = k;
  c.ns = strands == 3 ? 2 : 1;
  c.rev_only = strands == 2;
  return c;
}

// The offsets' rule at entry i of off[0 .. n_reads]: off[0] = 0, off[i] <= off[i + 1], off[n_reads]
// = n_bases.  Reads only off[i] and off[i + 1] (i < n_reads).
__host__ __device__ inline bool rq_off_ok_at(const int64_t* off, int64_t i, int64_t n_reads,
                                             int64_t n_bases) {
  const int64_t a = off[i];
  if (i == 0 && a != 0) return false;
  if (i == n_reads) return a == n_bases;
  return a <= off[i + 1];
}
inline ReadsCall reads_off_refusal(const int64_t* off, int64_t n_reads, int64_t n_bases) {
  for (int64_t i = 0; i <= n_reads; ++i)
    if (!rq_off_ok_at(off, i, n_reads, n_bases)) return reads_refusal(KMHG_EINVAL, RQ_OFF_TEXT);
  return ReadsCall{};
}

// Entries of the virtual window space.
__host__ __device__ inline int64_t rq_virtual(int64_t n_bases, int ns) { return n_bases * ns; }

// The last index r of a[lo .. hi] with a[r] <= q (lo when none is: a[lo] <= q is the caller's, for
// valid offsets a[0] = 0).  For q < n_bases this is the read that holds base q: empty reads before
// it share its offset and lose to it.  Never reads outside a[lo .. hi], whatever a holds.
__host__ __device__ inline int64_t rq_last_le(const int64_t* a, int64_t lo, int64_t hi, int64_t q) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (a[mid] <= q) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The window of a virtual entry.
struct RqWin {
  int64_t a = 0;               // the read's first base in seq
  int64_t len = 0;
  int64_t s = 0;               // 0-based window start in the strand's own coordinates
  bool rc = false;
};

// Entry v of read r = [a, b) (a = off[r], b = off[r + 1], found by rq_last_le over base v / ns).
// False where the offsets do not hold v's base inside [0, n_bases) -- broken offsets, which the
// device answers with its fault flag and no access outside the buffers.
__host__ __device__ inline bool rq_locate(int64_t v, int ns, bool rev_only, int64_t a, int64_t b,
                                          int64_t n_bases, RqWin& w) {
  const int64_t q = ns == 2 ? v >> 1 : v;
  if (a < 0 || b > n_bases || q < a || q >= b) return false;
  const int64_t len = b - a, u = v - a * ns;
  const bool second = u >= len;          // (only with ns = 2)
  w.a = a;
  w.len = len;
  w.s = second ? u - len : u;
  w.rc = ns == 2 ? second : rev_only;
  return true;
}

// The first entry of read r's strand (0 forward, 1 reverse, in a both-strands space).
__host__ __device__ inline int64_t rq_entry(int64_t a, int64_t len, int ns, bool second,
                                            int64_t s) {
  return a * ns + (second ? len : 0) + s;
}

__host__ __device__ inline bool rq_is_n(uint8_t c) { return (c | 0x20u) == 'n'; }   // LC(c) == 'n'
__host__ __device__ inline uint64_t rq_code(uint8_t c) { return (c >> 1) & 3u; }    // UPDATE_OFFSET

// Window s of a read of len bases rd[0 .. len) on one strand, by the reference's walk with the
// read as the whole sequence: a window exists iff s + k <= len, it holds no N, and it is not the
// dropped end window -- s + k == len with s == 0 or an N just before it.  rc: the window of
// rc(read), read from the forward bases: rc char p is the complement of rd[len - 1 - p] (code ^ 2,
// an N stays an N: kmhg_revcomp.h), so the char before rc window s is rd[len - s], and the
// dropped window s = len - k is the read's forward window 0, dropped iff len == k or rd[k] is N.
// Reads rd[0 .. len) only.
__host__ __device__ inline bool rq_window_key(const uint8_t* rd, int64_t len, int k, int64_t s,
                                              bool rc, uint64_t& key) {
  if (s < 0 || s + k > len) return false;
  if (s + k == len) {
    if (s == 0) return false;
    if (rq_is_n(rc ? rd[len - s] : rd[s - 1])) return false;
  }
  uint64_t x = 0;
  bool n = false;
  for (int i = 0; i < k; ++i) {
    const uint8_t c = rc ? rd[len - 1 - s - i] : rd[s + i];
    n |= rq_is_n(c);
    x = (x << 2) | (rq_code(c) ^ (rc ? 2u : 0u));
  }
  key = x;
  return !n;
}

// Rows are written into a guessed capacity before their number is known: one per virtual entry,
// an eighth more, and 64 (query_rows_guess's rule over the entries).
inline uint64_t rq_rows_guess(int64_t V) { return (uint64_t)V + ((uint64_t)V >> 3) + 64; }

// A row is four int32 (read, strand, i, j): row r at byte 16 r.
constexpr int RQ_ROW_INTS = 4;
inline uint64_t rq_rows_bytes(uint64_t H) { return H * (uint64_t)(RQ_ROW_INTS * sizeof(int32_t)); }
// A host matrix has int dimensions.
inline ReadsCall rq_fill_refusal(int64_t H) {
  if (H > (int64_t)INT32_MAX) return reads_refusal(KMHG_EOVERFLOW, "result has more than 2^31-1 rows");
  return ReadsCall{};
}

// ------------------------------------------------------------------ reads.kmer.vote
// A row votes for pos = j - i + k, the index position of base 1 of its strand's read (<= 0 when
// the read hangs over the index's start), in cell (strand, bin = floor(pos / band)).  Per read:
// the cell with the most votes, ties to the forward strand, then to the smaller bin.
constexpr int64_t VOTE_BAND_MAX = (int64_t)1 << 30;
constexpr int VOTE_COLS = 6;   // read, strand, pos, hits, second, total

inline ReadsCall vote_refusal(int64_t n_rows, int64_t n_reads, int k, int64_t band) {
  if (k < 1 || k > 31) return reads_refusal(KMHG_EINVAL, "k should be between 1 and 31");
  if (band < 1 || band > VOTE_BAND_MAX)
    return reads_refusal(KMHG_EINVAL, "band must be between 1 and 2^30");
  if (n_rows < 0 || n_reads < 0) return reads_refusal(KMHG_EINVAL, "negative row or read count");
  if (n_reads > RQ_MAX_READS)
    return reads_refusal(KMHG_EOVERFLOW, "more than 2^31-1 reads in one call: split the reads");
  if (n_rows > (int64_t)INT32_MAX)
    return reads_refusal(KMHG_EOVERFLOW, "more than 2^31-1 rows in one vote: split the rows");
  return ReadsCall{};
}

// floor(pos / band), toward minus infinity (band >= 1).
__host__ __device__ inline int64_t vote_bin(int64_t pos, int64_t band) {
  const int64_t q = pos / band;
  return q * band > pos ? q - 1 : q;
}

// The sort key of a row's cell: read (0-based, 31 bits) | strand (0 forward, 1 reverse) | the
// bin + 2^31 (32 bits: |pos| < 2^31 + 32, so every bin does fit).  Ascending keys are read, then
// forward first, then bin.
__host__ __device__ inline uint64_t vote_key(int64_t read0, bool reverse, int64_t bin) {
  return ((uint64_t)read0 << 33) | ((uint64_t)(reverse ? 1u : 0u) << 32) |
         (uint64_t)(uint32_t)(bin + ((int64_t)1 << 31));
}
__host__ __device__ inline int64_t vote_key_read0(uint64_t key) { return (int64_t)(key >> 33); }

// A cell's entry in its read's maximum: count (31 bits) over the INVERTED strand and bin, so the
// largest word is the most votes, then forward, then the smaller bin.  Never 0 for a count >= 1.
__host__ __device__ inline uint64_t vote_pack(uint32_t count, uint64_t key) {
  return ((uint64_t)count << 33) | (~key & 0x1FFFFFFFFull);
}
__host__ __device__ inline uint32_t vote_pack_count(uint64_t p) { return (uint32_t)(p >> 33); }
__host__ __device__ inline int32_t vote_pack_strand(uint64_t p) { return ((p >> 32) & 1u) ? 1 : -1; }
__host__ __device__ inline int64_t vote_pack_bin(uint64_t p) {
  return (int64_t)(uint32_t)~(uint32_t)p - ((int64_t)1 << 31);
}

}  // namespace kmhg
#pragma GCC visibility pop
