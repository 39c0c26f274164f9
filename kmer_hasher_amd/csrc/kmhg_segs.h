// kmhg_segs.h -- the pieces of the diagonal-segment pass that need no device (no HIP: any C++
// compiler; the kernels of kmhg_segs.hip include the same functions).
//
// seq.kmer.segs turns the (i, j) rows of a seq.kmer.pos result -- i, j >= 1, strictly ascending
// by (i, j) -- into maximal diagonal segments (i, j, len): (i + t, j + t) is a row for
// 0 <= t < len, (i - 1, j - 1) and (i + len, j + len) are not (include/kmhgpu.h).  Membership is
// decided from the rows alone, so every row is classified by two lookups:
//   start   (i - 1, j - 1) is not a row      end   (i + 1, j + 1) is not a row
// The wanted row, if present, lies just before (after) row r in the (i, j) order: behind the rest
// of window i - 1's hits and in front of the rest of window i's.  seg_find_back / seg_find_fwd
// therefore gallop away from r (1, 2, 4, ... rows) until they pass the target and bisect the last
// stride, O(log distance) reads instead of O(log n) over the whole matrix; the first probe is the
// neighbour row, which settles every single-hit window (the read run_start does).  Both stay
// inside [0, n) and terminate on ANY input, sorted or not.
//
// Starts and ends are then paired by sorting: seg_key orders by diagonal (j - i) first, then by
// i, and on one diagonal starts and ends alternate, so the m-th smallest start key and the m-th
// smallest end key bound the same segment and len = end.i - start.i + 1.  No lane walks a
// segment.
//
// R is any type with int32 members x (= i) and y (= j): int2 on the device.
// tools/asan/segs_check runs a host pass made of these functions against a set-based restatement
// under ASan + UBSan (tests/test_segs_host.py).
#pragma once
#include <stdint.h>

#include "kmhg_common.h"

namespace kmhg {

// The (i, j) order as one unsigned compare (i, j >= 1).
__host__ __device__ inline uint64_t seg_lex(int32_t i, int32_t j) {
  return ((uint64_t)(uint32_t)i << 32) | (uint32_t)j;
}
template <class R>
__host__ __device__ inline uint64_t seg_lex(const R& v) { return seg_lex(v.x, v.y); }

// Pairing key: the diagonal j - i, biased by 2^31 into a u32 (|j - i| <= 2^31 - 2), over i.
__host__ __device__ inline uint64_t seg_key(int32_t i, int32_t j) {
  const uint32_t d = (uint32_t)j - (uint32_t)i + 0x80000000u;
  return ((uint64_t)d << 32) | (uint32_t)i;
}
__host__ __device__ inline int32_t seg_key_i(uint64_t key) { return (int32_t)(uint32_t)key; }
__host__ __device__ inline int32_t seg_key_j(uint64_t key) {
  return (int32_t)((uint32_t)key + (uint32_t)(key >> 32) - 0x80000000u);
}
// Rows of the segment whose first row has key `start` and whose last row has key `end` (one
// diagonal, end.i >= start.i).
__host__ __device__ inline int32_t seg_len(uint64_t start, uint64_t end) {
  return (int32_t)((uint32_t)end - (uint32_t)start + 1u);
}

// Whether a row with seg_lex == target is among rows[0, r), all of which are expected below
// rows[r] (target < seg_lex(rows[r])).  Gallops backwards from r - 1.
template <class R>
__host__ __device__ inline bool seg_find_back(const R* rows, int64_t r, uint64_t target) {
  int64_t hi = r;                       // every probed row in [hi, r) is above the target
  int64_t lo = r - 1, step = 1;
  for (;;) {
    if (lo < 0) { lo = -1; break; }     // (row -1: below everything)
    const uint64_t v = seg_lex(rows[lo]);
    if (v == target) return true;
    if (v < target) break;
    hi = lo;
    lo -= step;
    step <<= 1;
  }
  while (hi - lo > 1) {                 // rows[lo] < target < rows[hi]
    const int64_t mid = lo + ((hi - lo) >> 1);
    const uint64_t v = seg_lex(rows[mid]);
    if (v == target) return true;
    if (v < target) lo = mid; else hi = mid;
  }
  return false;
}

// Whether a row with seg_lex == target is among rows(r, n) (target > seg_lex(rows[r])).  Gallops
// forwards from r + 1.
template <class R>
__host__ __device__ inline bool seg_find_fwd(const R* rows, int64_t r, int64_t n, uint64_t target) {
  int64_t lo = r;                       // every probed row in (r, lo] is below the target
  int64_t hi = r + 1, step = 1;
  for (;;) {
    if (hi >= n) { hi = n; break; }     // (row n: above everything)
    const uint64_t v = seg_lex(rows[hi]);
    if (v == target) return true;
    if (v > target) break;
    lo = hi;
    hi += step;
    step <<= 1;
  }
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const uint64_t v = seg_lex(rows[mid]);
    if (v == target) return true;
    if (v < target) lo = mid; else hi = mid;
  }
  return false;
}

// Row r's class: bit 0 = it starts a segment, bit 1 = it ends one, and the two input faults the
// pass reports: SEG_UNSORTED = the row before it is not below it, SEG_NONPOS = i < 1 or j < 1.
// A predecessor with a zero coordinate, or a successor past INT32_MAX, is never a row.
constexpr uint32_t SEG_START = 1, SEG_END = 2, SEG_UNSORTED = 4, SEG_NONPOS = 8;
template <class R>
__host__ __device__ inline uint32_t seg_classify(const R* rows, int64_t r, int64_t n) {
  const R v = rows[r];
  uint32_t c = 0;
  if (v.x < 1 || v.y < 1) return SEG_START | SEG_END | SEG_NONPOS;
  if (r > 0 && seg_lex(rows[r - 1]) >= seg_lex(v)) c |= SEG_UNSORTED;
  if (v.x == 1 || v.y == 1 || !seg_find_back(rows, r, seg_lex(v.x - 1, v.y - 1))) c |= SEG_START;
  if (v.x == INT32_MAX || v.y == INT32_MAX ||
      !seg_find_fwd(rows, r, n, seg_lex(v.x + 1, v.y + 1)))
    c |= SEG_END;
  return c;
}

}  // namespace kmhg
