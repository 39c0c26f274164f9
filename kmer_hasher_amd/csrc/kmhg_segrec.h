// kmhg_segrec.h -- the arithmetic of the row-free segment route that needs no device (no HIP: any
// C++ compiler; the kernels of kmhg_segrec.hip include the same functions).
//
// A probed query leaves one record per window s of [w0, w1) (put_qrec, kmhg_kernels.hip): its hit
// set P(s) is nothing (qrec[s] == 0), {qrec[s]} (one hit), or the ascending list
// positions[st, st + n) with {n, st} = qmulti[s] (SEGREC_MULTI).  Window s has i = w0 + s + kq and
// its rows are (i, j) for j in P(s), in the order (s, q) with q the index in the list.  The
// definition of kmhg_segs.h then reads, with the search in H sorted rows replaced by a search in
// one neighbour window's list:
//   hit (s, j) starts a segment  iff s == 0       or j == 1         or j - 1 is not in P(s - 1)
//   it ends one                  iff s == Nw - 1  or j == INT32_MAX or j + 1 is not in P(s + 1)
// No sequence character is compared: the reverse strand, a query k that is not the index k, N runs
// and the end-drop rule are whatever the records say, as in the rows route.
//
// Membership in a list gallops from a hint, the hit's own index q clamped to the neighbour list
// (segrec_find): in a homopolymer the neighbour list is the same array and j - 1 sits just before
// q, in a tandem repeat within one place of it, elsewhere lists are short -- O(log distance)
// reads, never O(log n) from scratch.  Like seg_find_back / seg_find_fwd it stays inside the list
// and terminates on ANY input, ascending or not.
//
// M is any type with u32 members x (= n) and y (= st): uint2 on the device.
// tools/asan/segrec_check runs a host pass made of these functions against a set-based restatement
// under ASan + UBSan (tests/test_segrec_host.py).
#pragma once
#include <stdint.h>

#include "../../include/kmhgpu.h"
#include "kmhg_common.h"
#include "kmhg_segs.h"

namespace kmhg {

constexpr uint32_t SEGREC_MULTI = 0x80000000u;   // QREC_MULTI of kmhg_kernels.hip (put_qrec)
// windows with at most this many hits are classified by their own lane (EMIT_DIRECT of Q_emit)
constexpr uint32_t SEGREC_DIRECT = 4;

// Whether `target` is among the ascending p[0, n); the search starts at p[min(hint, n - 1)] and
// gallops away from it (1, 2, 4, ... elements) until it passes the target, then bisects the last
// stride.
__host__ __device__ inline bool segrec_find(const int32_t* p, uint32_t n, uint32_t hint,
                                            int32_t target) {
  if (!n) return false;
  const int64_t h = hint < n ? hint : n - 1;
  int32_t v = p[h];
  if (v == target) return true;
  int64_t lo, hi, step = 1;
  if (v > target) {                     // backwards: every probed element in [hi, h] is above
    hi = h;
    lo = h - 1;
    for (;;) {
      if (lo < 0) { lo = -1; break; }   // (element -1: below everything)
      v = p[lo];
      if (v == target) return true;
      if (v < target) break;
      hi = lo;
      lo -= step;
      step <<= 1;
    }
  } else {                              // forwards: every probed element in [h, lo] is below
    lo = h;
    hi = h + 1;
    for (;;) {
      if (hi >= (int64_t)n) { hi = n; break; }   // (element n: above everything)
      v = p[hi];
      if (v == target) return true;
      if (v > target) break;
      lo = hi;
      hi += step;
      step <<= 1;
    }
  }
  while (hi - lo > 1) {                 // p[lo] < target < p[hi]
    const int64_t mid = lo + ((hi - lo) >> 1);
    v = p[mid];
    if (v == target) return true;
    if (v < target) lo = mid; else hi = mid;
  }
  return false;
}

// Whether j is a hit of window s: none, single or list.
template <class M>
__host__ __device__ inline bool segrec_has(const uint32_t* qrec, const M* qmulti,
                                           const int32_t* positions, int64_t s, uint32_t hint,
                                           int32_t j) {
  const uint32_t rec = qrec[s];
  if (rec != SEGREC_MULTI) return rec != 0u && (int32_t)rec == j;
  const M v = qmulti[s];
  return segrec_find(positions + v.y, v.x, hint, j);
}

// The class of hit j, the q-th of window s of Nw: SEG_START | SEG_END bits (kmhg_segs.h).  A
// predecessor j - 1 == 0, or a successor past INT32_MAX, is never a hit.
template <class M>
__host__ __device__ inline uint32_t segrec_classify(const uint32_t* qrec, const M* qmulti,
                                                    const int32_t* positions, int64_t Nw,
                                                    int64_t s, uint32_t q, int32_t j) {
  uint32_t c = 0;
  if (s == 0 || j == 1 || !segrec_has(qrec, qmulti, positions, s - 1, q, j - 1)) c |= SEG_START;
  if (s == Nw - 1 || j == INT32_MAX || !segrec_has(qrec, qmulti, positions, s + 1, q, j + 1))
    c |= SEG_END;
  return c;
}

// What the route refuses once the exact 64-bit totals are known (H > 0).  On every diagonal starts
// and ends alternate, so there are as many of each; the handle counts segments in an int32 range.
struct SegrecRefusal {
  int code;             // KMHG_OK: S = starts segments
  const char* text;
};
__host__ __device__ inline SegrecRefusal segrec_check_totals(uint64_t starts, uint64_t ends) {
  if (!starts || starts != ends) return {KMHG_EDEVICE, "segment starts and ends do not pair"};
  if (starts > (uint64_t)INT32_MAX)
    return {KMHG_EOVERFLOW, "result has more than 2^31-1 segments"};
  return {KMHG_OK, nullptr};
}

}  // namespace kmhg
