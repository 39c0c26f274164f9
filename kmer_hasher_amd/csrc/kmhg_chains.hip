// kmhg_chains.hip -- seq.kmer.chains on the device: the blocks {i, j, span, hits} of
// seq.kmer.blocks linked across diagonals into chains {i, j, i.end, j.end, hits, blocks}.
// Definition: include/kmhgpu.h; the arithmetic: kmhg_chains.h.
//
// The input is B blocks in (i, j) order; b = 0 .. B - 1 is that order.  (ei, ej) is a block's last
// row.  One lane per block unless said otherwise; tiles of TILE blocks, element e = j * BLOCK + t,
// as the segment and block passes.
//
//   C_keys     the input faults (order, a block's own fields) written to the host's record, and
//              the sort key {ei << 32 | b} of every block
//   sort       hipcub::DeviceRadixSort of the keys (distinct): the blocks' indices by ei
//   C_prep     rank r of the sorted order: ej of its block, so the scan below reads two
//              contiguous arrays; block b: its window [lo, hi) of the sorted order, two binary
//              searches (chain_window)
//   C_pred     one wave per block b: the window read 64 candidates per step, each lane keeping
//              the minimum key {cost << 32 | a} of the candidates it saw (chain_candidate), one
//              wave minimum at the end.  Lane 0 stores pred(b) and enters b in the contest for
//              that predecessor: a device-scope 64-bit atomicMin of {cost << 32 | b} into
//              child[a] (child: B u64, all ones before)
//   C_link     link a -> b survives iff child[pred(b)] names b: up[b] = a, else b itself.  So a
//              block has a link out iff its child word is not all ones
//   C_jump     pointer jumping in place, up[b] <- up^4[b], chain_rounds(B) launches: any value a
//              lane reads is an ancestor on b's path, every launch multiplies the distance a
//              pointer covers by at least 4, and the chain's first block is a fixed point, so
//              the end state does not depend on the order the lanes ran in
//   C_sum      per chain head: atomicAdd of the blocks' hits and of 1; the chain's last block
//              (no link out) alone writes (ei, ej)
//   C_count / scan / C_emit   the heads with hits >= min_hits counted per tile and ranked in
//              block order -- the (i, j) order of the chains' first blocks, no second sort: the
//              record of the p-th kept head goes to chain p, and p + 1 into cid[head]
//   C_member   chain[b] = cid[up[b]] (cid zeroed before: 0 for a dropped chain)
// Every reduction is an integer minimum or sum, so the result is the same bytes on every run.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include "kmhg_chains.h"
#include "kmhg_common.h"
#include "kmhg_device.h"
#include "kmhg_kernels.h"

namespace kmhg {

namespace {

constexpr int NW = BLOCK / 64;

// DPP move of a u64 for a minimum: lanes without a source, or in a row the row mask leaves out,
// read all ones
template <int CTRL, int ROWS>
__device__ __forceinline__ uint64_t dpp_u64_ones(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)(uint32_t)v, CTRL, ROWS, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)(uint32_t)(v >> 32), CTRL, ROWS, 0xf, false);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t min_u64(uint64_t a, uint64_t b) { return a < b ? a : b; }
// the minimum over the wave's 64 lanes (every lane active), in every lane: wave_incl_scan's
// DPP pattern with min for +
__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
  v = min_u64(v, dpp_u64_ones<0x111, 0xf>(v));   // row_shr:1
  v = min_u64(v, dpp_u64_ones<0x112, 0xf>(v));   // row_shr:2
  v = min_u64(v, dpp_u64_ones<0x114, 0xf>(v));   // row_shr:4
  v = min_u64(v, dpp_u64_ones<0x118, 0xf>(v));   // row_shr:8
  v = min_u64(v, dpp_u64_ones<0x142, 0xa>(v));   // row_bcast:15 into rows 1 and 3
  v = min_u64(v, dpp_u64_ones<0x143, 0xc>(v));   // row_bcast:31 into rows 2 and 3
  return lane63(v);
}

__device__ __forceinline__ uint32_t ld_relaxed32(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_relaxed32(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(BLOCK)
k_chains_keys(const int4* __restrict__ blocks, uint32_t B, uint64_t* __restrict__ keys,
              uint32_t* __restrict__ unsorted, uint32_t* __restrict__ bad) {
  const uint64_t b = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (b >= B) return;
  const int4 v = blocks[b];
  const int4 p = b ? blocks[b - 1] : v;
  const uint32_t f = chain_check_block(b != 0, p.x, p.y, v.x, v.y, v.z, v.w);
  if (f & CHAIN_UNSORTED) *unsorted = 1u;     // same value from every lane that sees one
  if (f & CHAIN_BAD_BLOCK) *bad = 1u;
  // (a faulty block's key is some u64 like any other: every index below stays in [0, B))
  keys[b] = chain_sort_key((int32_t)chain_end(v.x, v.z), (uint32_t)b);
}

__global__ void __launch_bounds__(BLOCK)
k_chains_prep(const int4* __restrict__ blocks, uint32_t B, const uint64_t* __restrict__ skey,
              uint32_t max_dist, int32_t* __restrict__ sej, uint2* __restrict__ win) {
  const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= B) return;
  const uint32_t a = chain_sort_key_index(skey[t]);
  // the keys carry the indices 0 .. B - 1, so a < B always; like the ranks of the emit passes the
  // index is still compared with its bound before it is used, and a rank whose index were out of
  // range gets the one ej no block can follow (gj < 0): every word of sej is defined
  int32_t ej = INT32_MAX;
  if (a < B) {
    const int4 v = blocks[a];
    ej = (int32_t)chain_end(v.y, v.z);
  }
  sej[t] = ej;
  uint32_t lo, hi;
  chain_window(skey, B, blocks[t].x, max_dist, &lo, &hi);
  win[t] = make_uint2(lo, hi);
}

__global__ void __launch_bounds__(BLOCK)
k_chains_pred(const int4* __restrict__ blocks, uint32_t B, const uint64_t* __restrict__ skey,
              const int32_t* __restrict__ sej, const uint2* __restrict__ win, uint32_t max_dist,
              uint32_t max_drift, uint64_t* __restrict__ pred, uint64_t* __restrict__ child) {
  const uint64_t b = (uint64_t)blockIdx.x * NW + (threadIdx.x >> 6);   // one wave per block
  if (b >= B) return;
  const int lane = lane_id();
  const int4 v = blocks[b];
  const uint2 w = win[b];                     // lo <= hi <= B (chain_window)
  uint64_t best = CHAIN_NONE;
  for (uint64_t r = (uint64_t)w.x + lane; r < w.y; r += 64) {
    const uint64_t k = skey[r];
    uint32_t cost;
    if (chain_candidate(chain_sort_key_end(k), sej[r], v.x, v.y, max_dist, max_drift, &cost))
      best = min_u64(best, chain_key(cost, chain_sort_key_index(k)));
  }
  best = wave_min(best);
  if (lane == 0) {
    pred[b] = best;
    const uint32_t a = chain_key_index(best);
    if (best != CHAIN_NONE && a < B)
      atomicMin((unsigned long long*)&child[a],
                (unsigned long long)chain_key(chain_key_cost(best), (uint32_t)b));
  }
}

__global__ void __launch_bounds__(BLOCK)
k_chains_link(uint32_t B, const uint64_t* __restrict__ pred, const uint64_t* __restrict__ child,
              uint32_t* __restrict__ up) {
  const uint64_t b = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (b >= B) return;
  const uint64_t p = pred[b];
  uint32_t h = (uint32_t)b;
  if (p != CHAIN_NONE) {
    const uint32_t a = chain_key_index(p);
    if (a < B && chain_key_index(child[a]) == (uint32_t)b) h = a;
  }
  up[b] = h;
}

__global__ void __launch_bounds__(BLOCK)
k_chains_jump(uint32_t B, uint32_t* __restrict__ up) {
  const uint64_t b = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (b >= B) return;
  uint32_t x = ld_relaxed32(&up[b]);          // (every value of up is in [0, B))
#pragma unroll
  for (int hop = 0; hop < 3; ++hop) x = ld_relaxed32(&up[x]);
  st_relaxed32(&up[b], x);
}

__global__ void __launch_bounds__(BLOCK)
k_chains_sum(const int4* __restrict__ blocks, uint32_t B, const uint32_t* __restrict__ up,
             const uint64_t* __restrict__ child, uint32_t* __restrict__ hits,
             uint32_t* __restrict__ count, int2* __restrict__ ends) {
  const uint64_t b = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (b >= B) return;
  const int4 v = blocks[b];
  const uint32_t h = up[b];
  atomicAdd(&hits[h], (uint32_t)v.w);
  atomicAdd(&count[h], 1u);
  if (child[b] == CHAIN_NONE)                 // the chain's last block: the only writer
    ends[h] = make_int2((int32_t)chain_end(v.x, v.z), (int32_t)chain_end(v.y, v.z));
}

__device__ __forceinline__ bool kept_head(const uint32_t* __restrict__ up,
                                          const uint32_t* __restrict__ hits, uint64_t b,
                                          uint32_t B, uint32_t min_hits) {
  return b < B && up[b] == (uint32_t)b && hits[b] >= min_hits;
}

__global__ void __launch_bounds__(BLOCK)
k_chains_count(uint32_t B, const uint32_t* __restrict__ up, const uint32_t* __restrict__ hits,
               uint32_t min_hits, uint64_t* __restrict__ tile_cnt) {
  __shared__ uint32_t wc[NW];
  const uint64_t t0 = (uint64_t)blockIdx.x * TILE;
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    const uint64_t b = t0 + (uint64_t)j * BLOCK + threadIdx.x;
    c += (uint32_t)__popcll(__ballot(kept_head(up, hits, b, B, min_hits)));
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
k_chains_emit(const int4* __restrict__ blocks, uint32_t B, const uint32_t* __restrict__ up,
              const uint32_t* __restrict__ hits, const uint32_t* __restrict__ count,
              const int2* __restrict__ ends, uint32_t min_hits,
              const uint64_t* __restrict__ tile_off, uint64_t C, int2* __restrict__ out,
              uint32_t* __restrict__ cid) {
  __shared__ uint64_t cw[WPT * NW + 1];
  const uint64_t t0 = (uint64_t)blockIdx.x * TILE;
  bool keep[WPT];
#pragma unroll
  for (int j = 0; j < WPT; ++j)
    keep[j] = kept_head(up, hits, t0 + (uint64_t)j * BLOCK + threadIdx.x, B, min_hits);
  uint64_t rk[WPT];
  tile_rank_at<WPT>(keep, rk, cw, tile_off[blockIdx.x]);
#pragma unroll
  for (int j = 0; j < WPT; ++j) {
    if (keep[j] && rk[j] < C) {               // (the rank against its bound before the store)
      const uint64_t b = t0 + (uint64_t)j * BLOCK + threadIdx.x;
      const int4 v = blocks[b];
      const int2 e = ends[b];
      int2* o = out + 3 * rk[j];
      o[0] = make_int2(v.x, v.y);
      o[1] = e;
      o[2] = make_int2((int32_t)hits[b], (int32_t)count[b]);
      cid[b] = (uint32_t)rk[j] + 1u;
    }
  }
}

__global__ void __launch_bounds__(BLOCK)
k_chains_member(uint32_t B, const uint32_t* __restrict__ up, const uint32_t* __restrict__ cid,
                int32_t* __restrict__ member) {
  const uint64_t b = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (b >= B) return;
  member[b] = (int32_t)cid[up[b]];
}

inline unsigned tiles_of(uint64_t n) { return (unsigned)((n + TILE - 1) / TILE); }
inline unsigned groups_of(uint64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

}  // namespace

void launch_chains_keys(const int32_t* blocks, uint32_t B, uint64_t* keys, uint32_t* unsorted,
                        uint32_t* bad, hipStream_t s) {
  hipLaunchKernelGGL(k_chains_keys, dim3(groups_of(B)), dim3(BLOCK), 0, s,
                     reinterpret_cast<const int4*>(blocks), B, keys, unsorted, bad);
}
hipError_t chains_sort_temp_bytes(uint32_t B, size_t* bytes) {
  return hipcub::DeviceRadixSort::SortKeys(nullptr, *bytes, (const uint64_t*)nullptr,
                                           (uint64_t*)nullptr, (int)B, 0, 64);
}
hipError_t launch_chains_sort(const uint64_t* keys, uint32_t B, uint64_t* skey, void* temp,
                              size_t temp_bytes, hipStream_t s) {
  size_t tb = temp_bytes;
  return hipcub::DeviceRadixSort::SortKeys(temp, tb, keys, skey, (int)B, 0, 64, s);
}
void launch_chains_prep(const int32_t* blocks, uint32_t B, const uint64_t* skey, uint32_t max_dist,
                        int32_t* sej, uint32_t* win, hipStream_t s) {
  hipLaunchKernelGGL(k_chains_prep, dim3(groups_of(B)), dim3(BLOCK), 0, s,
                     reinterpret_cast<const int4*>(blocks), B, skey, max_dist, sej,
                     reinterpret_cast<uint2*>(win));
}
void launch_chains_pred(const int32_t* blocks, uint32_t B, const uint64_t* skey, const int32_t* sej,
                        const uint32_t* win, uint32_t max_dist, uint32_t max_drift, uint64_t* pred,
                        uint64_t* child, hipStream_t s) {
  hipLaunchKernelGGL(k_chains_pred, dim3((unsigned)(((uint64_t)B + NW - 1) / NW)), dim3(BLOCK), 0,
                     s, reinterpret_cast<const int4*>(blocks), B, skey, sej,
                     reinterpret_cast<const uint2*>(win), max_dist, max_drift, pred, child);
}
void launch_chains_link(uint32_t B, const uint64_t* pred, const uint64_t* child, uint32_t* up,
                        hipStream_t s) {
  hipLaunchKernelGGL(k_chains_link, dim3(groups_of(B)), dim3(BLOCK), 0, s, B, pred, child, up);
}
void launch_chains_jump(uint32_t B, uint32_t* up, hipStream_t s) {
  hipLaunchKernelGGL(k_chains_jump, dim3(groups_of(B)), dim3(BLOCK), 0, s, B, up);
}
void launch_chains_sum(const int32_t* blocks, uint32_t B, const uint32_t* up, const uint64_t* child,
                       uint32_t* hits, uint32_t* count, int32_t* ends, hipStream_t s) {
  hipLaunchKernelGGL(k_chains_sum, dim3(groups_of(B)), dim3(BLOCK), 0, s,
                     reinterpret_cast<const int4*>(blocks), B, up, child, hits, count,
                     reinterpret_cast<int2*>(ends));
}
void launch_chains_count(uint32_t B, const uint32_t* up, const uint32_t* hits, uint32_t min_hits,
                         uint64_t* tile_cnt, hipStream_t s) {
  hipLaunchKernelGGL(k_chains_count, dim3(tiles_of(B)), dim3(BLOCK), 0, s, B, up, hits, min_hits,
                     tile_cnt);
}
void launch_chains_emit(const int32_t* blocks, uint32_t B, const uint32_t* up, const uint32_t* hits,
                        const uint32_t* count, const int32_t* ends, uint32_t min_hits,
                        const uint64_t* tile_off, uint64_t C, int32_t* out, uint32_t* cid,
                        hipStream_t s) {
  hipLaunchKernelGGL(k_chains_emit, dim3(tiles_of(B)), dim3(BLOCK), 0, s,
                     reinterpret_cast<const int4*>(blocks), B, up, hits, count,
                     reinterpret_cast<const int2*>(ends), min_hits, tile_off, C,
                     reinterpret_cast<int2*>(out), cid);
}
void launch_chains_member(uint32_t B, const uint32_t* up, const uint32_t* cid, int32_t* member,
                          hipStream_t s) {
  hipLaunchKernelGGL(k_chains_member, dim3(groups_of(B)), dim3(BLOCK), 0, s, B, up, cid, member);
}

}  // namespace kmhg
