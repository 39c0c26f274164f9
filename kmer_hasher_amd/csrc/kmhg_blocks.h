// kmhg_blocks.h -- the arithmetic of the block pass that needs no device (no HIP: any C++
// compiler; the kernels of kmhg_blocks.hip include the same functions).
//
// seq.kmer.blocks merges the maximal diagonal segments of some rows (kmhg_segs.h) across small
// gaps: on one diagonal, consecutive kept segments a, b with b.i - (a.i + a.len) <= max_gap belong
// to one block {i, j, span, hits} (include/kmhgpu.h has the definition).  The segment pass leaves
// every segment as two pairing keys (seg_key: diagonal, then i), the one of its first row and the
// one of its last, both sorted -- so the segments of one diagonal are neighbours in ascending i,
// and whether segment m opens a block is decided from the end key of m - 1 and the start key of m
// alone (blk_head).  Block ids, spans and hits then come from scans; no lane walks a diagonal.
//
// All coordinates are in [1, 2^31 - 1] and the gap is taken in u32, so nothing overflows.
// tools/asan/blocks_check runs a host pass made of these functions against a restatement that
// walks each diagonal, under ASan + UBSan (tests/test_blocks_host.py).
#pragma once
#include <stdint.h>

#include "kmhg_segs.h"

namespace kmhg {

// Whether two pairing keys lie on one diagonal.
__host__ __device__ inline bool blk_same_diag(uint64_t a, uint64_t b) {
  return (uint32_t)(a >> 32) == (uint32_t)(b >> 32);
}
// Windows between a segment whose last row has key `end` and the next segment of its diagonal,
// whose first row has key `start`: start.i - (end.i + 1), >= 1 for maximal segments.
__host__ __device__ inline uint32_t blk_gap(uint64_t end, uint64_t start) {
  return (uint32_t)start - (uint32_t)end - 1u;
}
// Windows from a block's first row (key `start`) to its last (key `end`), both inclusive.
__host__ __device__ inline int32_t blk_span(uint64_t start, uint64_t end) {
  return seg_len(start, end);
}
// max_gap as the u32 the gaps are compared with: no gap exceeds 2^31 - 3, so every larger
// max_gap means "any gap".
__host__ __device__ inline uint32_t blk_gap_limit(int64_t max_gap) {
  return max_gap > (int64_t)0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)max_gap;
}
// Whether the segment starting at `start` opens a block, given the end key of the kept segment
// before it in the (diagonal, i) order (the first segment of all always does).
__host__ __device__ inline bool blk_head(uint64_t prev_end, uint64_t start, uint32_t gap_limit) {
  return !blk_same_diag(prev_end, start) || blk_gap(prev_end, start) > gap_limit;
}

}  // namespace kmhg
