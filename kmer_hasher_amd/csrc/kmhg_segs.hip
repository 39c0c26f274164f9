// kmhg_segs.hip -- seq.kmer.segs on the device: a query's (i, j) rows as maximal diagonal
// segments (i, j, len).  Definition and the search / pairing arithmetic: kmhg_segs.h.
//
//   S_classify  one lane per row, tiles of TILE rows (element e = j * BLOCK + t, as the run
//               kernels): start / end by seg_classify -- the neighbour row first, a galloping
//               search only where a window has several hits -- kept as one ballot word per 64
//               rows each (2 bits per row, so the searches run once), the tile's start and end
//               counts packed in one u64 {ends << 32 | starts}, and the two input faults
//               (rows not ascending, a coordinate < 1) written to the host's record
//   scan        launch_scan_u64 over the packed counts: both exclusive scans in one pass
//               (n_rows < 2^31, so neither half carries into the other)
//   S_emit      starts and ends compacted in row order from the ballot words: the pairing key
//               (seg_key: diagonal, then i) of every start with its rank among the starts, and of
//               every end
//   sort        hipcub::DeviceRadixSort of the start keys (rank as payload) and of the end keys;
//               keys are distinct.  The m-th start and the m-th end bound one segment
//   S_pair      (i, j, len) scattered to the start's rank: the segments in the (i, j) order of
//               their first rows, with no lane walking a segment
//   S_filter    min_len > 1 only: count / scan / emit of the segments with len >= min_len
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include "kmhg_common.h"
#include "kmhg_device.h"
#include "kmhg_kernels.h"
#include "kmhg_segs.h"

namespace kmhg {

namespace {

constexpr int NW = BLOCK / 64;

__global__ void __launch_bounds__(BLOCK)
k_segs_classify(const int2* __restrict__ rows, uint64_t n, uint64_t* __restrict__ smask,
                uint64_t* __restrict__ emask, uint64_t* __restrict__ tile_cnt,
                uint32_t* __restrict__ unsorted, uint32_t* __restrict__ nonpos) {
  __shared__ uint64_t wc[NW];
  const uint64_t t0 = (uint64_t)blockIdx.x * TILE;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  uint64_t cnt = 0;
  uint32_t fault = 0;
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const uint64_t r = t0 + (uint64_t)j * BLOCK + threadIdx.x;
    const uint32_t c = r < n ? seg_classify(rows, (int64_t)r, (int64_t)n) : 0u;
    const uint64_t ms = __ballot(c & SEG_START), me = __ballot(c & SEG_END);
    fault |= c;
    if (lane == 0) {                    // (the mask arrays cover whole tiles)
      const uint64_t w = (t0 + (uint64_t)j * BLOCK + (uint64_t)wave * 64) >> 6;
      smask[w] = ms;
      emask[w] = me;
    }
    cnt += (uint64_t)__popcll(ms) | ((uint64_t)__popcll(me) << 32);
  }
  if (fault & SEG_UNSORTED) *unsorted = 1u;   // same value from every lane that sees one
  if (fault & SEG_NONPOS) *nonpos = 1u;
  if (lane == 0) wc[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) t += wc[w];
    tile_cnt[blockIdx.x] = t;
  }
}

__global__ void __launch_bounds__(BLOCK)
k_segs_emit(const int2* __restrict__ rows, uint64_t n, const uint64_t* __restrict__ smask,
            const uint64_t* __restrict__ emask, const uint64_t* __restrict__ tile_off,
            uint64_t* __restrict__ skey, uint32_t* __restrict__ srank,
            uint64_t* __restrict__ ekey) {
  __shared__ uint64_t cws[WPT * NW + 1], cwe[WPT * NW + 1];
  const uint64_t t0 = (uint64_t)blockIdx.x * TILE;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  bool st[WPT], en[WPT];
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const uint64_t w = (t0 + (uint64_t)j * BLOCK + (uint64_t)wave * 64) >> 6;
    st[j] = (smask[w] >> lane) & 1u;
    en[j] = (emask[w] >> lane) & 1u;
  }
  const uint64_t off = tile_off[blockIdx.x];
  uint64_t rs[WPT], re[WPT];
  tile_rank_at<WPT>(st, rs, cws, off & 0xFFFFFFFFull);
  tile_rank_at<WPT>(en, re, cwe, off >> 32);
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    if (st[j] || en[j]) {               // (mask bits are set for rows < n only)
      const int2 v = rows[t0 + (uint64_t)j * BLOCK + threadIdx.x];
      const uint64_t key = seg_key(v.x, v.y);
      if (st[j]) {
        skey[rs[j]] = key;
        srank[rs[j]] = (uint32_t)rs[j];
      }
      if (en[j]) ekey[re[j]] = key;
    }
  }
}

__global__ void __launch_bounds__(BLOCK)
k_segs_pair(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ srank,
            const uint64_t* __restrict__ ekey, uint64_t S, int32_t* __restrict__ out) {
  const uint64_t m = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (m >= S) return;
  const uint64_t a = skey[m], b = ekey[m];
  int32_t* o = out + 3 * (uint64_t)srank[m];
  o[0] = seg_key_i(a);
  o[1] = seg_key_j(a);
  o[2] = seg_len(a, b);
}

__global__ void __launch_bounds__(BLOCK)
k_segs_filter_count(const int32_t* __restrict__ segs, uint64_t S, int32_t min_len,
                    uint64_t* __restrict__ tile_cnt) {
  __shared__ uint32_t wc[NW];
  const uint64_t t0 = (uint64_t)blockIdx.x * TILE;
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const uint64_t m = t0 + (uint64_t)j * BLOCK + threadIdx.x;
    c += (uint32_t)__popcll(__ballot(m < S && segs[3 * m + 2] >= min_len));
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
k_segs_filter_emit(const int32_t* __restrict__ segs, uint64_t S, int32_t min_len,
                   const uint64_t* __restrict__ tile_off, int32_t* __restrict__ out) {
  __shared__ uint64_t cw[WPT * NW + 1];
  const uint64_t t0 = (uint64_t)blockIdx.x * TILE;
  bool keep[WPT];
  int32_t len[WPT];
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const uint64_t m = t0 + (uint64_t)j * BLOCK + threadIdx.x;
    len[j] = m < S ? segs[3 * m + 2] : 0;
    keep[j] = len[j] >= min_len;        // (min_len >= 1)
  }
  uint64_t rk[WPT];
  tile_rank_at<WPT>(keep, rk, cw, tile_off[blockIdx.x]);
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    if (keep[j]) {
      const int32_t* v = segs + 3 * (t0 + (uint64_t)j * BLOCK + threadIdx.x);
      int32_t* o = out + 3 * rk[j];
      o[0] = v[0];
      o[1] = v[1];
      o[2] = len[j];
    }
  }
}

inline unsigned tiles_of(uint64_t n) { return (unsigned)((n + TILE - 1) / TILE); }

}  // namespace

void launch_segs_classify(const int2* rows, uint64_t n, uint64_t* smask, uint64_t* emask,
                          uint64_t* tile_cnt, uint32_t* unsorted, uint32_t* nonpos,
                          hipStream_t s) {
  hipLaunchKernelGGL(k_segs_classify, dim3(tiles_of(n)), dim3(BLOCK), 0, s, rows, n, smask, emask,
                     tile_cnt, unsorted, nonpos);
}
void launch_segs_emit(const int2* rows, uint64_t n, const uint64_t* smask, const uint64_t* emask,
                      const uint64_t* tile_off, uint64_t* skey, uint32_t* srank, uint64_t* ekey,
                      hipStream_t s) {
  hipLaunchKernelGGL(k_segs_emit, dim3(tiles_of(n)), dim3(BLOCK), 0, s, rows, n, smask, emask,
                     tile_off, skey, srank, ekey);
}
hipError_t segs_sort_temp_bytes(uint64_t S, size_t* bytes) {
  size_t a = 0, b = 0;
  hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const uint64_t*)nullptr,
                                                    (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                                    (uint32_t*)nullptr, (int)S, 0, 64);
  if (e != hipSuccess) return e;
  e = hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                        (int)S, 0, 64);
  *bytes = a > b ? a : b;
  return e;
}
hipError_t launch_segs_sort(const uint64_t* skey, const uint32_t* srank, const uint64_t* ekey,
                            uint64_t S, uint64_t* skey_out, uint32_t* srank_out,
                            uint64_t* ekey_out, void* temp, size_t temp_bytes, hipStream_t s) {
  size_t tb = temp_bytes;
  hipError_t e = hipcub::DeviceRadixSort::SortPairs(temp, tb, skey, skey_out, srank, srank_out,
                                                    (int)S, 0, 64, s);
  if (e != hipSuccess) return e;
  tb = temp_bytes;
  return hipcub::DeviceRadixSort::SortKeys(temp, tb, ekey, ekey_out, (int)S, 0, 64, s);
}
void launch_segs_pair(const uint64_t* skey, const uint32_t* srank, const uint64_t* ekey,
                      uint64_t S, int32_t* out, hipStream_t s) {
  hipLaunchKernelGGL(k_segs_pair, dim3((unsigned)((S + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s,
                     skey, srank, ekey, S, out);
}
void launch_segs_filter_count(const int32_t* segs, uint64_t S, int32_t min_len,
                              uint64_t* tile_cnt, hipStream_t s) {
  hipLaunchKernelGGL(k_segs_filter_count, dim3(tiles_of(S)), dim3(BLOCK), 0, s, segs, S, min_len,
                     tile_cnt);
}
void launch_segs_filter_emit(const int32_t* segs, uint64_t S, int32_t min_len,
                             const uint64_t* tile_off, int32_t* out, hipStream_t s) {
  hipLaunchKernelGGL(k_segs_filter_emit, dim3(tiles_of(S)), dim3(BLOCK), 0, s, segs, S, min_len,
                     tile_off, out);
}

}  // namespace kmhg
