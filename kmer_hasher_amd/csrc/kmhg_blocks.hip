// kmhg_blocks.hip -- seq.kmer.blocks on the device: the diagonal segments of a query's rows
// merged across gaps of at most max_gap windows into blocks (i, j, span, hits).  Definition:
// include/kmhgpu.h; the arithmetic: kmhg_blocks.h.
//
// The input is what the segment pass sorts (kmhg_segs.hip): segment m's start key, end key and
// the rank of its first row among all starts, for the S segments in (diagonal, i) order.  Tiles of
// TILE segments, element e = j * BLOCK + t as there.
//
//   B_filter   min_len > 1 only: count / scan / emit of the segments with len >= min_len, the
//              three arrays compacted in that order (a dropped segment's neighbours become
//              neighbours, so the gap between them spans it)
//   B_heads    segment m opens a block if m == 0 or blk_head(end[m - 1], start[m]); per tile the
//              head count and the sum of len packed in one u64 {len << 32 | heads}, so one
//              launch_scan_u64 gives both exclusive prefixes.  heads < 2^31 never carries into
//              the upper half; the len half is a sum modulo 2^32 (what leaves bit 63 is dropped):
//              the lens sum to the hit total, which the row-free route takes beyond 2^32, and
//              only differences of two prefixes are used -- a block's hits, below 2^31 because
//              a block lies on one diagonal -- which are exact modulo 2^32
//   B_mark     the same pair scanned inside the tile: block id = heads before m.  A head writes
//              its block's start key, rank and the len prefix before it; a tail (the last segment,
//              or the one before the next head) the end key and the len prefix after it
//   B_place    one lane per block: hits = the difference of the two prefixes; a block with
//              hits >= min_hits puts id + 1 into slot[rank of its first row] (slot: S u32, zeroed)
//   B_order    count / scan / emit of the non-zero slots in rank order -- the (i, j) order of the
//              blocks' first rows, with no sort by value: {i, j, span, hits} of the block named by
//              the p-th non-zero slot goes to record p
// Every element is written by exactly one lane, so the result is the same bytes on every run.
#include <hip/hip_runtime.h>
#include "kmhg_blocks.h"
#include "kmhg_common.h"
#include "kmhg_device.h"
#include "kmhg_kernels.h"

namespace kmhg {

namespace {

constexpr int NW = BLOCK / 64;

__global__ void __launch_bounds__(BLOCK)
k_blocks_filter_count(const uint64_t* __restrict__ skey, const uint64_t* __restrict__ ekey,
                      uint64_t S, int32_t min_len, uint64_t* __restrict__ tile_cnt) {
  __shared__ uint32_t wc[NW];
  const uint64_t t0 = (uint64_t)blockIdx.x * TILE;
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const uint64_t m = t0 + (uint64_t)j * BLOCK + threadIdx.x;
    c += (uint32_t)__popcll(__ballot(m < S && seg_len(skey[m], ekey[m]) >= min_len));
  }
  if (lane_id() == 0) wc[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) t += wc[w];
    tile_cnt[blockIdx.x] = t;
  }
}

__global__ void __launch_bounds__(BLOCK)
k_blocks_filter_emit(const uint64_t* __restrict__ skey, const uint64_t* __restrict__ ekey,
                     const uint32_t* __restrict__ srank, uint64_t S, int32_t min_len,
                     const uint64_t* __restrict__ tile_off, uint64_t* __restrict__ fskey,
                     uint64_t* __restrict__ fekey, uint32_t* __restrict__ frank) {
  __shared__ uint64_t cw[WPT * NW + 1];
  const uint64_t t0 = (uint64_t)blockIdx.x * TILE;
  bool keep[WPT];
  uint64_t a[WPT], b[WPT];
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const uint64_t m = t0 + (uint64_t)j * BLOCK + threadIdx.x;
    a[j] = m < S ? skey[m] : 0;
    b[j] = m < S ? ekey[m] : 0;
    keep[j] = m < S && seg_len(a[j], b[j]) >= min_len;
  }
  uint64_t rk[WPT];
  tile_rank_at<WPT>(keep, rk, cw, tile_off[blockIdx.x]);
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    if (keep[j]) {
      fskey[rk[j]] = a[j];
      fekey[rk[j]] = b[j];
      frank[rk[j]] = srank[t0 + (uint64_t)j * BLOCK + threadIdx.x];
    }
  }
}

// {len << 32 | head} of segment m < K
__device__ __forceinline__ uint64_t head_and_len(const uint64_t* __restrict__ skey,
                                                 const uint64_t* __restrict__ ekey, uint64_t m,
                                                 uint32_t gap_limit) {
  const uint64_t a = skey[m];
  const bool head = m == 0 || blk_head(ekey[m - 1], a, gap_limit);
  return ((uint64_t)(uint32_t)seg_len(a, ekey[m]) << 32) | (head ? 1u : 0u);
}

__global__ void __launch_bounds__(BLOCK)
k_blocks_heads(const uint64_t* __restrict__ skey, const uint64_t* __restrict__ ekey, uint64_t K,
               uint32_t gap_limit, uint64_t* __restrict__ tile_cnt) {
  __shared__ uint64_t wc[NW];
  const uint64_t t0 = (uint64_t)blockIdx.x * TILE;
  uint64_t v = 0;
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const uint64_t m = t0 + (uint64_t)j * BLOCK + threadIdx.x;
    if (m < K) v += head_and_len(skey, ekey, m, gap_limit);
  }
  v = wave_sum(v);                      // (heads never carry up; the len half is modulo 2^32)
  if (lane_id() == 0) wc[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) t += wc[w];
    tile_cnt[blockIdx.x] = t;
  }
}

__global__ void __launch_bounds__(BLOCK)
k_blocks_mark(const uint64_t* __restrict__ skey, const uint64_t* __restrict__ ekey,
              const uint32_t* __restrict__ srank, uint64_t K, uint32_t gap_limit,
              const uint64_t* __restrict__ tile_off, uint64_t* __restrict__ bstart,
              uint64_t* __restrict__ bend, uint32_t* __restrict__ brank,
              uint32_t* __restrict__ bpre, uint32_t* __restrict__ bpost) {
  __shared__ uint64_t lds[5];
  const uint64_t t0 = (uint64_t)blockIdx.x * TILE;
  uint64_t base = tile_off[blockIdx.x];
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const uint64_t m = t0 + (uint64_t)j * BLOCK + threadIdx.x;
    const uint64_t v = m < K ? head_and_len(skey, ekey, m, gap_limit) : 0;
    uint64_t tot;
    const uint64_t ex = base + block_excl_scan(v, lds, tot);
    base += tot;
    if (m < K) {
      const uint32_t head = (uint32_t)v & 1u;
      const uint32_t heads_before = (uint32_t)ex, len_before = (uint32_t)(ex >> 32);
      const uint64_t e = ekey[m];
      if (head) {
        bstart[heads_before] = skey[m];
        brank[heads_before] = srank[m];
        bpre[heads_before] = len_before;
      }
      if (m + 1 == K || blk_head(e, skey[m + 1], gap_limit)) {
        const uint32_t b = heads_before + head - 1u;   // (segment 0 is a head: never below 0)
        bend[b] = e;
        bpost[b] = len_before + (uint32_t)(v >> 32);
      }
    }
  }
}

__global__ void __launch_bounds__(BLOCK)
k_blocks_place(const uint64_t* __restrict__ total, const uint32_t* __restrict__ brank,
               const uint32_t* __restrict__ bpre, const uint32_t* __restrict__ bpost,
               uint32_t min_hits, uint32_t* __restrict__ slot) {
  const uint64_t b = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (b >= (*total & 0xFFFFFFFFull)) return;          // the scan's total: {len << 32 | heads}
  if (bpost[b] - bpre[b] >= min_hits) slot[brank[b]] = (uint32_t)b + 1u;
}

__global__ void __launch_bounds__(BLOCK)
k_blocks_order_count(const uint32_t* __restrict__ slot, uint64_t S,
                     uint64_t* __restrict__ tile_cnt) {
  __shared__ uint32_t wc[NW];
  const uint64_t t0 = (uint64_t)blockIdx.x * TILE;
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const uint64_t r = t0 + (uint64_t)j * BLOCK + threadIdx.x;
    c += (uint32_t)__popcll(__ballot(r < S && slot[r] != 0u));
  }
  if (lane_id() == 0) wc[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) t += wc[w];
    tile_cnt[blockIdx.x] = t;
  }
}

__global__ void __launch_bounds__(BLOCK)
k_blocks_order_emit(const uint32_t* __restrict__ slot, uint64_t S,
                    const uint64_t* __restrict__ tile_off, const uint64_t* __restrict__ bstart,
                    const uint64_t* __restrict__ bend, const uint32_t* __restrict__ bpre,
                    const uint32_t* __restrict__ bpost, int4* __restrict__ out) {
  __shared__ uint64_t cw[WPT * NW + 1];
  const uint64_t t0 = (uint64_t)blockIdx.x * TILE;
  bool has[WPT];
  uint32_t id[WPT];
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const uint64_t r = t0 + (uint64_t)j * BLOCK + threadIdx.x;
    id[j] = r < S ? slot[r] : 0u;
    has[j] = id[j] != 0u;
  }
  uint64_t rk[WPT];
  tile_rank_at<WPT>(has, rk, cw, tile_off[blockIdx.x]);
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    if (has[j]) {
      const uint32_t b = id[j] - 1u;
      const uint64_t a = bstart[b];
      out[rk[j]] = make_int4(seg_key_i(a), seg_key_j(a), blk_span(a, bend[b]),
                             (int32_t)(bpost[b] - bpre[b]));
    }
  }
}

inline unsigned tiles_of(uint64_t n) { return (unsigned)((n + TILE - 1) / TILE); }

}  // namespace

void launch_blocks_filter_count(const uint64_t* skey, const uint64_t* ekey, uint64_t S,
                                int32_t min_len, uint64_t* tile_cnt, hipStream_t s) {
  hipLaunchKernelGGL(k_blocks_filter_count, dim3(tiles_of(S)), dim3(BLOCK), 0, s, skey, ekey, S,
                     min_len, tile_cnt);
}
void launch_blocks_filter_emit(const uint64_t* skey, const uint64_t* ekey, const uint32_t* srank,
                               uint64_t S, int32_t min_len, const uint64_t* tile_off,
                               uint64_t* fskey, uint64_t* fekey, uint32_t* frank, hipStream_t s) {
  hipLaunchKernelGGL(k_blocks_filter_emit, dim3(tiles_of(S)), dim3(BLOCK), 0, s, skey, ekey, srank,
                     S, min_len, tile_off, fskey, fekey, frank);
}
void launch_blocks_heads(const uint64_t* skey, const uint64_t* ekey, uint64_t K,
                         uint32_t gap_limit, uint64_t* tile_cnt, hipStream_t s) {
  hipLaunchKernelGGL(k_blocks_heads, dim3(tiles_of(K)), dim3(BLOCK), 0, s, skey, ekey, K,
                     gap_limit, tile_cnt);
}
void launch_blocks_mark(const uint64_t* skey, const uint64_t* ekey, const uint32_t* srank,
                        uint64_t K, uint32_t gap_limit, const uint64_t* tile_off, uint64_t* bstart,
                        uint64_t* bend, uint32_t* brank, uint32_t* bpre, uint32_t* bpost,
                        hipStream_t s) {
  hipLaunchKernelGGL(k_blocks_mark, dim3(tiles_of(K)), dim3(BLOCK), 0, s, skey, ekey, srank, K,
                     gap_limit, tile_off, bstart, bend, brank, bpre, bpost);
}
void launch_blocks_place(const uint64_t* total, uint64_t K, const uint32_t* brank,
                         const uint32_t* bpre, const uint32_t* bpost, uint32_t min_hits,
                         uint32_t* slot, hipStream_t s) {
  hipLaunchKernelGGL(k_blocks_place, dim3((unsigned)((K + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s,
                     total, brank, bpre, bpost, min_hits, slot);
}
void launch_blocks_order_count(const uint32_t* slot, uint64_t S, uint64_t* tile_cnt,
                               hipStream_t s) {
  hipLaunchKernelGGL(k_blocks_order_count, dim3(tiles_of(S)), dim3(BLOCK), 0, s, slot, S,
                     tile_cnt);
}
void launch_blocks_order_emit(const uint32_t* slot, uint64_t S, const uint64_t* tile_off,
                              const uint64_t* bstart, const uint64_t* bend, const uint32_t* bpre,
                              const uint32_t* bpost, int32_t* out, hipStream_t s) {
  hipLaunchKernelGGL(k_blocks_order_emit, dim3(tiles_of(S)), dim3(BLOCK), 0, s, slot, S, tile_off,
                     bstart, bend, bpre, bpost, reinterpret_cast<int4*>(out));
}

}  // namespace kmhg
