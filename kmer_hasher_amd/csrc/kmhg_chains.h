// kmhg_chains.h -- the arithmetic of the chain pass that needs no device (no HIP: any C++
// compiler; the kernels of kmhg_chains.hip include the same functions).
//
// seq.kmer.chains links the blocks {i, j, span, hits} of seq.kmer.blocks across diagonals
// (include/kmhgpu.h has the definition).  Block b's last row is (ei, ej) = (i + span - 1,
// j + span - 1).  Block a may precede block b when the gaps gi = i_b - ei_a - 1 and
// gj = j_b - ej_a - 1 are both >= 0, max(gi, gj) <= max_dist and |gj - gi| <= max_drift
// (chain_candidate); the link costs gi + gj.  Every choice is the minimum of a u64 key
// {cost << 32 | block index} (chain_key), so ties go to the lower index and a minimum over any
// grouping of the candidates is the same value.  gi >= 0 and gi <= max_dist bound ei_a to
// [i_b - 1 - max_dist, i_b - 1]: with the blocks' indices sorted by ei (chain_sort_key) the
// candidates of b lie in one window of that order, found by two binary searches
// (chain_window).
//
// All coordinates are in [1, 2^31 - 1]: a gap is at most 2^31 - 3, a cost below 2^32, and the
// differences are taken in int64, so nothing overflows.  tools/asan/chains_check runs a host pass
// made of these functions against an O(B^2) restatement, under ASan + UBSan
// (tests/test_chains_host.py).
#pragma once
#include <stdint.h>

#include "../../include/kmhgpu.h"
#include "kmhg_common.h"

namespace kmhg {

constexpr uint64_t CHAIN_NONE = ~0ull;      // no predecessor / no child (no key is all ones)

// max_dist / max_drift as the u32 the gaps are compared with: no gap exceeds 2^31 - 3, so every
// larger value means "any".
__host__ __device__ inline uint32_t chain_limit(int64_t v) {
  return v > (int64_t)0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)v;
}
// min_hits as the u32 the hit sums are compared with: a chain's hits stay below 2^31, so every
// larger min_hits keeps no chain.
__host__ __device__ inline uint32_t chain_min_hits(int64_t v) {
  return v > (int64_t)0x7FFFFFFFll ? 0x80000000u : (uint32_t)v;
}

struct ChainRefusal {
  int code;
  const char* text;
};
// kmhg_blocks_chains' refusals of its parameters, before any device work and in this order.
inline ChainRefusal chain_check_params(int64_t max_dist, int64_t max_drift, int64_t min_hits) {
  if (max_dist < 0) return {KMHG_EINVAL, "max_dist must not be negative"};
  if (max_drift < 0) return {KMHG_EINVAL, "max_drift must not be negative"};
  if (min_hits < 1) return {KMHG_EINVAL, "min_hits must be a positive integer"};
  return {KMHG_OK, ""};
}
inline ChainRefusal chain_check_count(int64_t n_blocks) {
  if (n_blocks < 0 || n_blocks > (int64_t)0x7FFFFFFFll) return {KMHG_EINVAL, "bad block count"};
  return {KMHG_OK, ""};
}

// The last row's coordinate of a block that starts at `start` and spans `span` windows.
__host__ __device__ inline int64_t chain_end(int32_t start, int32_t span) {
  return (int64_t)start + span - 1;
}

// The faults of block b = {i, j, span, hits} given the block before it in the input (has_prev):
// the input must ascend strictly by (i, j); a block has i, j >= 1, 1 <= hits <= span and its last
// row within 2^31 - 1.
constexpr uint32_t CHAIN_UNSORTED = 1u, CHAIN_BAD_BLOCK = 2u;
__host__ __device__ inline uint32_t chain_check_block(bool has_prev, int32_t pi, int32_t pj,
                                                      int32_t i, int32_t j, int32_t span,
                                                      int32_t hits) {
  uint32_t f = 0;
  if (has_prev && !(pi < i || (pi == i && pj < j))) f |= CHAIN_UNSORTED;
  if (i < 1 || j < 1 || span < 1 || hits < 1 || hits > span ||
      chain_end(i, span) > (int64_t)0x7FFFFFFFll || chain_end(j, span) > (int64_t)0x7FFFFFFFll)
    f |= CHAIN_BAD_BLOCK;
  return f;
}
inline ChainRefusal chain_fault_refusal(uint32_t faults) {
  if (faults & CHAIN_UNSORTED) return {KMHG_EINVAL, "blocks are not in ascending (i, j) order"};
  if (faults & CHAIN_BAD_BLOCK)
    return {KMHG_EINVAL, "blocks must have i, j >= 1, 1 <= hits <= span and ends within 2^31 - 1"};
  return {KMHG_OK, ""};
}

// {ei << 32 | b}: the blocks' indices ordered by the i of their last row.  Keys are distinct.
__host__ __device__ inline uint64_t chain_sort_key(int32_t ei, uint32_t b) {
  return ((uint64_t)(uint32_t)ei << 32) | b;
}
__host__ __device__ inline uint32_t chain_sort_key_index(uint64_t key) { return (uint32_t)key; }
__host__ __device__ inline int32_t chain_sort_key_end(uint64_t key) {
  return (int32_t)(uint32_t)(key >> 32);
}

// Whether a block whose last row is (ei_a, ej_a) may precede one whose first row is (i_b, j_b);
// *cost <- gi + gj where it may.
__host__ __device__ inline bool chain_candidate(int32_t ei_a, int32_t ej_a, int32_t i_b,
                                                int32_t j_b, uint32_t max_dist,
                                                uint32_t max_drift, uint32_t* cost) {
  const int64_t gi = (int64_t)i_b - ei_a - 1, gj = (int64_t)j_b - ej_a - 1;
  if (gi < 0 || gj < 0) return false;
  const int64_t dist = gi > gj ? gi : gj, drift = gi > gj ? gi - gj : gj - gi;
  if (dist > (int64_t)max_dist || drift > (int64_t)max_drift) return false;
  *cost = (uint32_t)(gi + gj);
  return true;
}

// {cost << 32 | index}: what predecessors (index = a) and children (index = b) are chosen by.
__host__ __device__ inline uint64_t chain_key(uint32_t cost, uint32_t index) {
  return ((uint64_t)cost << 32) | index;
}
__host__ __device__ inline uint32_t chain_key_index(uint64_t key) { return (uint32_t)key; }
__host__ __device__ inline uint32_t chain_key_cost(uint64_t key) { return (uint32_t)(key >> 32); }

// The first r in [0, n) with keys[r] >= key, n if there is none (keys ascending).
__host__ __device__ inline uint32_t chain_lower_bound(const uint64_t* keys, uint32_t n,
                                                      uint64_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// The window [*lo, *hi) of the sorted keys that holds every block a with
// i_b - 1 - max_dist <= ei_a <= i_b - 1: all candidates of a block starting at row i_b.
__host__ __device__ inline void chain_window(const uint64_t* keys, uint32_t n, int32_t i_b,
                                             uint32_t max_dist, uint32_t* lo, uint32_t* hi) {
  const int64_t first = (int64_t)i_b - 1 - (int64_t)max_dist;
  *lo = chain_lower_bound(keys, n, chain_sort_key((int32_t)(first > 0 ? first : 0), 0u));
  *hi = chain_lower_bound(keys, n, chain_sort_key(i_b, 0u));
}

// Pointer-jumping rounds after which every block of a path of at most n blocks points at the
// path's first block, when a round multiplies the distance a pointer covers by 4.
__host__ __device__ inline int chain_rounds(uint64_t n) {
  int r = 0;
  for (uint64_t reach = 1; reach < n; reach *= 4) ++r;
  return r;
}

}  // namespace kmhg
